"""Arbitrary bytes in everything the Python layer hands the library uninitialised.

The library's contract is "kernels only, no memset": hs_forward / hs_backward and the other entry points get workspaces and
output tensors with whatever the allocator left in them, and must write every word before they read it (DESIGN.md 4.21 lists
who does that, region by region).  Every such buffer of the Python layer comes from torch.empty, torch.empty_like or
Tensor.new_empty; `poisoned` replaces the three for the duration of a `with` block so that each DEVICE tensor they return is
filled with a pattern first, and records every fill: a test compares a run under a pattern with the run under "zero" bit for
bit, and asserts from the records that the buffers it means were really filled (a refactor that allocates another way must
fail the test, not make it vacuous).  torch.zeros and the like are left alone: those buffers are initialised on purpose.

    with poisoned(monkeypatch, "ff") as session:
        out = run()
    session.require("casualhdrsplat_amd.rasterizer", roles=("geom", "binning", "image", "bwd", "flat_gradients"))

Not a conftest and not a fixture file: tests import it.
"""
from __future__ import annotations

import contextlib
import sys
from dataclasses import dataclass

import numpy as np
import torch

# Look-back status words (csrc/binning.hip).  Radix passes: one u32 per (pass, block, digit), flag << 30 | count (kStAgg =
# 1 << 30, kStIncl = 2 << 30, kStMask = 2^30 - 1).  Chained scan of the pair emission: one u64 per 256-instance block,
# flag << 62 | pairs (kScAgg = 1 << 62, kScIncl = 2 << 62, kScPoison = 3 << 62).  status_k / status64_k: flag k with an
# all-ones count in every word of that width (read at the other width, a status64_k word is flag 3 | all ones in its low
# half and flag k | all ones in its high half; a status_k pair is flag k with a count of 60 ones).
_ST_COUNT32, _ST_COUNT64 = (1 << 30) - 1, (1 << 62) - 1

FIXED = {
    "zero": b"\x00" * 8,
    "ff": b"\xff" * 8,
    "a5": b"\xa5" * 8,
    "one": (1).to_bytes(4, "little") * 2,
    "nan": (0x7FC00000).to_bytes(4, "little") * 2,
}
for _k in range(4):
    FIXED[f"status_{_k}"] = ((_k << 30) | _ST_COUNT32).to_bytes(4, "little") * 2
    FIXED[f"status64_{_k}"] = ((_k << 62) | _ST_COUNT64).to_bytes(8, "little")
PATTERNS = tuple(FIXED) + ("random", "stale")


def _as_bytes(t: torch.Tensor) -> torch.Tensor:
    """The storage bytes of a contiguous tensor, as a 1-D uint8 view."""
    if not t.is_contiguous():
        raise ValueError("poison: only contiguous tensors can be filled byte by byte")
    return t.reshape(-1).view(torch.uint8)


def tiled(src: torch.Tensor, n: int) -> torch.Tensor:
    """`src` (1-D uint8, at least one byte) repeated or cut to n bytes."""
    if src.numel() >= n:
        return src[:n]
    return src.repeat((n + src.numel() - 1) // src.numel())[:n]


def fill_(t: torch.Tensor, pattern: str, seed: int = 0, stale: torch.Tensor | None = None) -> torch.Tensor:
    """Fill `t` (any dtype, contiguous) with `pattern`, byte for byte, in place.  "random": bytes of a generator seeded with
    `seed` (on t's device); "stale": the bytes of `stale` (any tensor), tiled or cut to t's size."""
    if t.numel() == 0:
        return t
    b = _as_bytes(t)
    n = b.numel()
    if pattern in FIXED:
        if len(set(FIXED[pattern])) == 1:
            b.fill_(FIXED[pattern][0])
        else:
            b.copy_(tiled(torch.frombuffer(bytearray(FIXED[pattern]), dtype=torch.uint8).to(b.device), n))
    elif pattern == "random":
        g = torch.Generator(device=b.device)
        g.manual_seed(0x5EED + seed)
        b.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, device=b.device, generator=g))
    elif pattern == "stale":
        if stale is None or stale.numel() == 0:
            raise ValueError("poison: pattern 'stale' needs the bytes of an earlier buffer")
        b.copy_(tiled(_as_bytes(stale.detach()).to(b.device), n))
    else:
        raise ValueError(f"poison: unknown pattern {pattern!r} (known: {PATTERNS})")
    return t


@dataclass
class Fill:
    shape: tuple
    dtype: torch.dtype
    nbytes: int
    module: str          # __name__ of the module whose code asked for the tensor
    role: str            # rasterizer._empty's buffer name, else "<function>#<n-th request of that function in the session>"
    pattern: str
    stale_role: str | None = None   # "stale": the role of the earlier buffer whose bytes went in


class Session:
    """What one `poisoned` block filled.  `kept` (keep=True): role -> the filled tensor itself, so that a later block can use
    the bytes the library LEFT in it as its "stale" pattern."""

    def __init__(self, pattern, stale_from=None, keep=False, include_cpu=False):
        if pattern not in PATTERNS:
            raise ValueError(f"poison: unknown pattern {pattern!r} (known: {PATTERNS})")
        if pattern == "stale" and not (isinstance(stale_from, Session) and stale_from.kept):
            raise ValueError("poison: pattern 'stale' needs stale_from = a Session of an earlier block run with keep=True")
        self.pattern, self.stale_from, self.keep, self.include_cpu = pattern, stale_from, keep, include_cpu
        self.fills: list[Fill] = []
        self.kept: dict[str, torch.Tensor] = {}
        self._per_function: dict = {}

    # -- the hook --
    def _caller(self, depth: int):
        f = sys._getframe(depth)
        module, func = f.f_globals.get("__name__", "?"), f.f_code.co_name
        if func == "_empty" and isinstance(f.f_locals.get("name"), str):   # rasterizer._empty(shape, dtype, dev, name)
            return module, f.f_locals["name"]
        k = self._per_function.get((module, func), 0)
        self._per_function[(module, func)] = k + 1
        return module, f"{func}#{k}"

    def source_for(self, key: str):
        """Of a session run with keep=True: (key, tensor) of the buffer a later buffer of role `key` ("<module>:<role>")
        inherits its stale bytes from -- the buffer of the same role where there was one, else the largest one kept."""
        if key not in self.kept:
            key = max(self.kept, key=lambda k: (self.kept[k].numel() * self.kept[k].element_size(), k))
        return key, self.kept[key]

    def _touch(self, t, depth=3):
        if not isinstance(t, torch.Tensor) or t.numel() == 0 or not t.is_contiguous():
            return t
        if t.device.type == "cpu" and not self.include_cpu:
            return t
        if t.device.type == "meta":
            return t
        module, role = self._caller(depth)
        src_role = None
        if self.pattern == "stale":
            src_role, src = self.stale_from.source_for(f"{module}:{role}")
            fill_(t, "stale", stale=src)
        else:
            fill_(t, self.pattern, seed=len(self.fills))
        self.fills.append(Fill(tuple(t.shape), t.dtype, t.numel() * t.element_size(), module, role, self.pattern, src_role))
        if self.keep:
            self.kept[f"{module}:{role}"] = t
        return t

    # -- what tests ask --
    def of(self, module: str) -> list[Fill]:
        return [f for f in self.fills if f.module == module]

    def roles(self, module: str) -> list[str]:
        return [f.role for f in self.of(module)]

    def require(self, module: str, roles=(), at_least: int = 0) -> list[Fill]:
        """The fills requested by `module`; asserts that every role in `roles` is among them and that there are at least
        `at_least` -- the proof that the call under test really received poisoned buffers."""
        got = self.of(module)
        have = {f.role for f in got}
        missing = [r for r in roles if r not in have]
        assert not missing, f"{module}: buffers {missing} did not come through torch.empty* (filled: {sorted(have)})"
        assert len(got) >= max(at_least, 1 if not roles else 0), (module, len(got), at_least)
        return got


@contextlib.contextmanager
def poisoned(monkeypatch, pattern: str, stale_from: Session | None = None, keep: bool = False, include_cpu: bool = False):
    """Inside the block torch.empty, torch.empty_like and Tensor.new_empty fill every device tensor they return with
    `pattern` (PATTERNS) and record the fill; on leaving it the three are what they were.  Yields the Session.
    `stale_from`: the Session of an earlier block run with keep=True (pattern "stale": a buffer starts with the bytes the
    buffer of the same role held when that block ended).  `include_cpu`: fill host tensors too (the helper's own test)."""
    session = Session(pattern, stale_from, keep, include_cpu)
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def p_empty(*args, **kwargs):
        return session._touch(empty(*args, **kwargs))

    def p_empty_like(*args, **kwargs):
        return session._touch(empty_like(*args, **kwargs))

    def p_new_empty(self, *args, **kwargs):
        return session._touch(new_empty(self, *args, **kwargs))

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", p_empty)
        m.setattr(torch, "empty_like", p_empty_like)
        m.setattr(torch.Tensor, "new_empty", p_new_empty)
        yield session


def bytes_of(x) -> bytes:
    """The bytes of a tensor / array (NaN payloads included): what "bit for bit" compares."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return _as_bytes(x).numpy().tobytes() if x.numel() else b""
    return np.ascontiguousarray(x).tobytes()
