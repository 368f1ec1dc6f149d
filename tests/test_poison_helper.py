"""tests/poison.py on CPU tensors: the three callables are replaced inside the block and only there, every tensor they return
carries the pattern, every fill is recorded with its caller, and a `stale` block starts from the bytes an earlier block left."""
import numpy as np
import pytest
import torch

import poison


def _alloc():
    a = torch.empty(3, 5, dtype=torch.float32)
    b = torch.empty_like(torch.zeros(7, dtype=torch.int32))
    c = torch.zeros(2, dtype=torch.int64).new_empty((4,))
    d = torch.empty(0)
    return a, b, c, d


def _u32(t):
    return np.frombuffer(poison.bytes_of(t), dtype=np.uint32)


@pytest.mark.parametrize("pattern", [p for p in poison.PATTERNS if p != "stale"])
def test_fills_records_and_restores(monkeypatch, pattern):
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poison.poisoned(monkeypatch, pattern, include_cpu=True) as s:
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
        a, b, c, d = _alloc()
        z = torch.zeros(4)          # initialised on purpose: not the hook's business
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert "new_empty" not in torch.Tensor.__dict__ or torch.Tensor.__dict__["new_empty"] is before[2]
    assert not z.any() and d.numel() == 0
    want = {"zero": 0, "ff": 0xFFFFFFFF, "a5": 0xA5A5A5A5, "one": 1, "nan": 0x7FC00000,
            "status_0": 0x3FFFFFFF, "status_1": 0x7FFFFFFF, "status_2": 0xBFFFFFFF, "status_3": 0xFFFFFFFF}
    for t in (a, b, c):
        w = _u32(t)
        if pattern in want:
            assert (w == want[pattern]).all(), (pattern, hex(int(w[0])))
        elif pattern.startswith("status64_"):
            k = int(pattern[-1])
            q = np.frombuffer(poison.bytes_of(t)[:len(w) // 2 * 8], dtype=np.uint64)
            assert (q == np.uint64((k << 62) | ((1 << 62) - 1))).all()
            assert (q >> np.uint64(62) == k).all() and w[0] == 0xFFFFFFFF
        else:   # random: seeded -- neither constant nor the same in two buffers, and the same again in a second block
            assert len(set(w.tolist())) > 1
    if pattern == "nan":
        assert torch.isnan(a).all()
    assert [(f.shape, f.dtype, f.nbytes, f.module, f.pattern) for f in s.fills] == [
        ((3, 5), torch.float32, 60, __name__, pattern), ((7,), torch.int32, 28, __name__, pattern),
        ((4,), torch.int64, 32, __name__, pattern)]
    assert s.roles(__name__) == ["_alloc#0", "_alloc#1", "_alloc#2"]
    assert len(s.require(__name__, roles=("_alloc#1",), at_least=3)) == 3
    with pytest.raises(AssertionError):
        s.require(__name__, roles=("geom",))
    with pytest.raises(AssertionError):
        s.require("casualhdrsplat_amd.rasterizer")
    if pattern == "random":
        with poison.poisoned(monkeypatch, pattern, include_cpu=True):
            a2, b2, _, _ = _alloc()
        assert poison.bytes_of(a2) == poison.bytes_of(a) and poison.bytes_of(b2) == poison.bytes_of(b)
        assert poison.bytes_of(a)[:28] != poison.bytes_of(b)


def test_host_tensors_are_left_alone_by_default(monkeypatch):
    with poison.poisoned(monkeypatch, "ff") as s:
        _alloc()
    assert s.fills == []


def test_rasterizer_buffers_are_recorded_by_name(monkeypatch):
    """rasterizer._empty(shape, dtype, dev, name): the role of such a buffer is its name."""
    from casualhdrsplat_amd import rasterizer
    with poison.poisoned(monkeypatch, "a5", include_cpu=True) as s:
        t = rasterizer._empty((2, 3), torch.float32, torch.device("cpu"), "geom")
    assert (_u32(t) == 0xA5A5A5A5).all()
    assert [(f.module, f.role) for f in s.fills] == [("casualhdrsplat_amd.rasterizer", "geom")]
    s.require("casualhdrsplat_amd.rasterizer", roles=("geom",))


def test_stale_takes_the_bytes_the_earlier_block_left(monkeypatch):
    with pytest.raises(ValueError):
        poison.Session("stale")
    with poison.poisoned(monkeypatch, "zero", keep=True, include_cpu=True) as first:
        a, b, c, _ = _alloc()
    a.copy_(torch.arange(15, dtype=torch.float32).reshape(3, 5))      # what "the library" left in the first buffer
    b.fill_(7)
    c.fill_(-1)                                                       # (the largest buffer: 32 bytes ... a's 60 is larger)
    with poison.poisoned(monkeypatch, "stale", stale_from=first, include_cpu=True) as s:
        small = torch.empty(4, dtype=torch.float32)                   # another function: no such role -> the largest kept
        a2, b2, _, _ = _alloc()
        big = torch.empty(40, dtype=torch.float32)
    assert poison.bytes_of(a2) == poison.bytes_of(a) and poison.bytes_of(b2) == poison.bytes_of(b)      # same role, same size
    assert poison.bytes_of(small) == poison.bytes_of(a)[:16]                                           # truncated
    assert poison.bytes_of(big) == (poison.bytes_of(a) * 3)[:160]                                      # tiled
    assert [f.stale_role for f in s.fills] == [f"{__name__}:_alloc#0", f"{__name__}:_alloc#0", f"{__name__}:_alloc#1",
                                               f"{__name__}:_alloc#2", f"{__name__}:_alloc#0"]


def test_fill_rejects_what_it_does_not_know():
    with pytest.raises(ValueError):
        poison.fill_(torch.zeros(4), "nonsense")
    with pytest.raises(ValueError):
        poison.fill_(torch.zeros(4), "stale")
    with pytest.raises(ValueError):
        poison.Session("nonsense")
