"""tests/guard_bands.py on CPU tensors (the device check is injectable): what the GPU guard tests rely on."""
import pytest
import torch

from tests import guard_bands as GB

EVERY = dict(is_device=lambda t: True)
SMALL = dict(EVERY, band=1024)        # (a short band where the test walks it byte by byte)


def test_shapes_dtypes_and_contiguity_are_preserved():
    with GB.guarded(**EVERY) as s:
        cases = [torch.empty(3, 5), torch.empty((), dtype=torch.float32), torch.empty(0, 7), torch.empty(2, 0, 3),
                 torch.empty(13, dtype=torch.uint8), torch.empty(4, 3, dtype=torch.float64),
                 torch.empty(5, dtype=torch.int32), torch.empty(6, dtype=torch.int64), torch.empty(7, dtype=torch.bool),
                 torch.empty(3, 3, dtype=torch.float16), torch.empty_like(torch.zeros(2, 9, dtype=torch.bfloat16))]
        want = [((3, 5), torch.float32), ((), torch.float32), ((0, 7), torch.float32), ((2, 0, 3), torch.float32),
                ((13,), torch.uint8), ((4, 3), torch.float64), ((5,), torch.int32), ((6,), torch.int64),
                ((7,), torch.bool), ((3, 3), torch.float16), ((2, 9), torch.bfloat16)]
        for t, (shape, dtype) in zip(cases, want):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
            assert t.data_ptr() % 16 == 0 or t.numel() == 0
        # zero-byte tensors pass through; everything else is in the registry, once (zeros(2, 9) and its empty_like: two)
        assert len(s.registry) == len(cases) - 2 + 1
        assert len(GB.seen(shape=(), dtype=torch.float32)) == 1 and GB.seen(shape=())[0].nbytes == 4
        assert len(GB.seen(nbytes=13)) == 1 and not GB.seen(shape=(0, 7))
        # uint8 viewed as float32, as the library's workspaces are carved
        ws = torch.empty(64, dtype=torch.uint8)
        f = ws.view(torch.float32)
        assert f.shape == (16,) and f.is_contiguous()
        f.fill_(1.5)
        GB.assert_intact("views")
    assert not GB.damaged()


def test_contents_of_zeros_full_and_ones_are_preserved():
    with GB.guarded(**EVERY):
        z = torch.zeros(5, 3)
        zl = torch.zeros_like(torch.empty(4, dtype=torch.int32))
        f = torch.full((2, 3), 7.5)
        fl = torch.full_like(torch.empty(3, dtype=torch.int64), -3)
        o = torch.ones(6, dtype=torch.bool)
        ol = torch.ones_like(torch.empty(2, 2, dtype=torch.float64))
        s0 = torch.zeros((), dtype=torch.int64)
        GB.assert_intact("contents")
    assert torch.equal(z, torch.tensor(0.0).expand(5, 3)) and int(zl.abs().sum()) == 0 and zl.dtype == torch.int32
    assert bool((f == 7.5).all()) and f.shape == (2, 3)
    assert bool((fl == -3).all()) and fl.dtype == torch.int64
    assert bool(o.all()) and o.dtype == torch.bool and bool((ol == 1.0).all()) and ol.dtype == torch.float64
    assert int(s0) == 0 and s0.shape == ()


def test_the_bands_hold_the_pattern_and_read_as_nan_and_minus_one():
    with GB.guarded(**SMALL) as s:
        t = torch.empty(4, dtype=torch.float32)
        e = s.registry[0]
        assert e.big.numel() % GB.GRANULE == 0 and e.big.numel() >= 2 * 1024 + 16
        assert bool((e.big[:1024] == 0xFF).all()) and bool((e.big[1024 + 16:] == 0xFF).all())
        assert bool(torch.isnan(e.big[:1024].view(torch.float32)).all())
        assert bool(torch.isnan(e.big[:1024].view(torch.float16)).all())
        assert bool(torch.isnan(e.big[:1024].view(torch.bfloat16)).all())
        assert bool((e.big[:1024].view(torch.int32) == -1).all()) and bool((e.big[:1024].view(torch.int64) == -1).all())
        assert t.data_ptr() == e.big.data_ptr() + 1024
    with GB.guarded(pattern=0xA5, **SMALL) as s:
        torch.empty(3)
        assert bool((s.registry[0].big[:1024] == 0xA5).all())
        GB.assert_intact("other pattern")


def test_empty_bodies_hold_the_pattern_unless_asked_otherwise():
    with GB.guarded(**SMALL) as s:
        e, el = torch.empty(7, 3), torch.empty_like(torch.zeros(5, dtype=torch.int32))
        z = torch.zeros(4)
        assert bool(torch.isnan(e).all()) and bool((el == -1).all()) and bool((z == 0).all())
        GB.assert_intact("poisoned bodies")
    with GB.guarded(poison_bodies=False, **SMALL) as s:
        torch.empty(7, 3).fill_(1.0)
        e = s.registry[0]
        assert bool((e.big[:1024] == 0xFF).all()) and bool((e.big[1024 + 84:] == 0xFF).all())
        GB.assert_intact("plain bodies")


def test_the_default_band_is_one_mebibyte_on_the_allocators_granule():
    assert GB.G_BYTES == 1 << 20 and GB.G_BYTES % 512 == 0
    with GB.guarded(**EVERY) as s:
        t = torch.empty(5, dtype=torch.uint8)
        e = s.registry[0]
        assert t.data_ptr() - e.big.data_ptr() == GB.G_BYTES and e.big.numel() == 2 * GB.G_BYTES + 512


@pytest.mark.parametrize("where", ["before", "after", "far_before", "far_after", "both"])
def test_a_one_byte_overrun_is_reported_with_its_band_and_offset(where):
    with GB.guarded(**SMALL) as s:
        torch.empty(8)                                        # an untouched neighbour
        t = torch.empty(3, 5, dtype=torch.float32)            # 60 bytes: the trailing band starts off the 16-byte grid
        torch.zeros(9, dtype=torch.int32)
        e = s.registry[1]
        n = 60
        assert e.nbytes == n
        spots = {"before": [-1], "after": [n], "far_before": [-1024], "far_after": [e.big.numel() - 1024 - 1],
                 "both": [-7, -2, n + 3, n + 500]}[where]
        for off in spots:
            e.big[1024 + off] = 0
        t.fill_(2.0)                                          # writes inside the body are nobody's business
        d = GB.damaged()
        bands = sorted({x["band"] for x in d})
        assert bands == {"before": ["leading"], "far_before": ["leading"], "after": ["trailing"],
                         "far_after": ["trailing"], "both": ["leading", "trailing"]}[where]
        for x in d:
            assert x["shape"] == (3, 5) and x["dtype"] == torch.float32 and x["nbytes"] == n
            assert "test_a_one_byte_overrun" in x["site"]
            mine = [o for o in spots if (o < 0) == (x["band"] == "leading")]
            assert (x["first"], x["last"]) == (min(mine), max(mine))
        with pytest.raises(AssertionError, match=r"overrun-case.*\n.*\[3, 5\]"):
            GB.assert_intact("overrun-case")
    assert len(GB.damaged()) == len(d)        # still answerable after the `with`


def test_a_write_that_equals_the_pattern_is_the_one_thing_a_byte_band_cannot_see():
    """(why the GPU tests also compare every result with the unguarded run, and why a second pattern exists)"""
    with GB.guarded(**SMALL) as s:
        torch.empty(4)
        s.registry[0].big[1024 + 16] = 0xFF
        assert not GB.damaged()
    with GB.guarded(pattern=0x5A, **SMALL) as s:
        torch.empty(4)
        s.registry[0].big[1024 + 16] = 0xFF
        assert [d["first"] for d in GB.damaged()] == [16]


def test_an_untouched_run_reports_nothing():
    with GB.guarded(**EVERY):
        a = torch.zeros(100, 3)
        b = torch.empty_like(a)
        b.copy_(a + 1)
        c = GB.guard(torch.arange(12, dtype=torch.float64).reshape(3, 4))
        c.mul_(2)
        assert GB.damaged() == []
        GB.assert_intact("clean")
    assert torch.equal(c, 2 * torch.arange(12, dtype=torch.float64).reshape(3, 4))


def test_guard_rehomes_an_existing_tensor_with_its_bits():
    x = torch.randn(7, 3)
    x[2, 1] = float("nan")
    leaf = torch.randn(5, requires_grad=True)
    with GB.guarded(**EVERY) as s:
        gx = GB.guard(x)
        gl = GB.guard(leaf)
        assert GB.guard(None) is None
        assert torch.equal(gx.view(torch.int32), x.view(torch.int32)) and gx.data_ptr() != x.data_ptr()
        assert gl.requires_grad and gl.is_leaf and torch.equal(gl.detach(), leaf.detach())
        (gl * 2).sum().backward()
        assert torch.equal(gl.grad, torch.full((5,), 2.0))
        assert [e.how for e in s.registry[:2]] == ["guard", "guard"]
        assert s.registry[0].site == "test_guard_rehomes_an_existing_tensor_with_its_bits"
    with pytest.raises(RuntimeError, match="outside"):
        GB.guard(x)


def test_what_passes_through_untouched():
    with GB.guarded() as s:                                   # the real device check: CPU tensors are left alone
        t = torch.empty(4, 4)
        assert not s.registry and t.shape == (4, 4)
    transposed = torch.randn(4, 6).t()
    with GB.guarded(**EVERY) as s:
        nc = torch.empty_like(transposed)                     # preserve_format: a non-contiguous result
        assert not nc.is_contiguous() and not s.registry
        rg = torch.zeros(3, requires_grad=True)
        assert rg.is_leaf and rg.requires_grad and not s.registry
        dst = torch.Tensor()
        torch.zeros(3, out=dst)
        assert not s.registry


def test_allocators_are_restored_also_after_an_exception():
    before = {n: getattr(torch, n) for n in GB.PATCHED}
    with pytest.raises(ZeroDivisionError):
        with GB.guarded(**EVERY):
            assert all(getattr(torch, n) is not before[n] for n in GB.PATCHED)
            1 / 0
    assert all(getattr(torch, n) is before[n] for n in GB.PATCHED)
    with GB.guarded(**EVERY):
        pass
    assert all(getattr(torch, n) is before[n] for n in GB.PATCHED)


def test_nested_use_is_refused():
    before = torch.empty
    with GB.guarded(**EVERY):
        inner = torch.empty
        with pytest.raises(RuntimeError, match="already active"):
            with GB.guarded(**EVERY):
                pass
        assert torch.empty is inner                           # the refusal left the outer session in place
        assert tuple(torch.empty(2).shape) == (2,)
    assert torch.empty is before


def test_shortchange_moves_the_trailing_band_into_the_body():
    with GB.guarded(shortchange=((4, 6), 4), **SMALL) as s:
        a = torch.empty(4, 6)
        b = torch.empty(4, 6)                                  # only the first match is shortened
        assert a.shape == (4, 6) and [e.nbytes for e in s.registry] == [92, 96]
        assert not GB.damaged()
        a.fill_(1.0)                                          # the "kernel" writes all 24 floats
        b.fill_(1.0)
        d = GB.damaged()
        assert len(d) == 1 and d[0]["band"] == "trailing" and d[0]["first"] - d[0]["nbytes"] == 0
        assert d[0]["last"] - d[0]["nbytes"] == 3 and d[0]["shape"] == (4, 6)


def test_release_drops_the_registry():
    with GB.guarded(**EVERY) as s:
        torch.empty(3)
    assert len(s.registry) == 1
    GB.release()
    assert not s.registry
    with pytest.raises(RuntimeError, match="no guarded"):
        GB.damaged()
