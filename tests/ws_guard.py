"""A workspace with guard bands on both sides: the caller-supplied block of a `lrx_*` entry planted inside one larger uint8 buffer, so that a
test can see a kernel write outside the bytes its `*_workspace_bytes` declared, and can hand the entry a block of chosen (dirty) content.
Device-agnostic: the buffer lives wherever `device` says (the host tests use CPU tensors).

    g = Guarded(need, device)       # [guard | need bytes | guard]
    g.fill(0xFF); g.arm()           # dirty inner block, position-dependent pattern in the guards
    plant(index, g)                 # index._ws = g.ws
    ... the call under test ...
    assert g.check().numel() == 0   # no guard byte changed
    assert_planted(index, g)        # the call really ran in g.ws (a too-small block is silently replaced by the wrappers)"""
from __future__ import annotations

import torch

GUARD = 1 << 20


def _pattern(offsets: torch.Tensor) -> torch.Tensor:
    """The guard byte at each (int64) offset: a mix of the offset's bytes with an odd multiplier -- it differs between neighbouring offsets
    (the low byte advances by an odd step) and no memset, word fill or copy of a neighbouring region reproduces it."""
    x = offsets * 167 + (offsets >> 8) * 59 + (offsets >> 16) * 31 + 0x5B
    return (x & 0xFF).to(torch.uint8)


class Guarded:
    def __init__(self, need: int, device, guard: int = GUARD):
        need, guard = int(need), int(guard)
        if guard <= 0 or guard % 4096 != 0:
            raise ValueError(f"guard={guard} must be a positive multiple of 4096 (the inner block keeps the 256-byte alignment the plans assume)")
        if need < 0:
            raise ValueError(f"need={need} < 0")
        self.need, self.guard = need, guard
        # (a device allocation starts on a 512-byte boundary at least, and guard is a multiple of 4096: the inner block is 256-byte aligned)
        self.buf = torch.empty(guard + need + guard, dtype=torch.uint8, device=device)
        self.ws = self.buf[guard:guard + need]
        self._want = None

    def view(self, need: int) -> torch.Tensor:
        """The first `need` bytes of the inner block (a smaller call planted at the same start)."""
        if not 0 <= need <= self.need:
            raise ValueError(f"view({need}) outside the inner block of {self.need} bytes")
        return self.buf[self.guard:self.guard + need]

    def fill(self, pattern):
        """pattern: a byte (int), or a uint8 tensor of at most `need` bytes copied to the start of the inner block."""
        if isinstance(pattern, torch.Tensor):
            p = pattern.reshape(-1)
            if p.dtype != torch.uint8 or p.numel() > self.need:
                raise ValueError("fill: a uint8 tensor of at most `need` bytes")
            self.ws[:p.numel()].copy_(p)
        else:
            self.ws.fill_(int(pattern) & 0xFF)
        return self

    def _guards(self):
        return self.buf[:self.guard], self.buf[self.guard + self.need:]

    def arm(self):
        lo, hi = self._guards()
        dev = self.buf.device
        lo.copy_(_pattern(torch.arange(0, self.guard, dtype=torch.int64, device=dev)))
        hi.copy_(_pattern(torch.arange(self.guard + self.need, 2 * self.guard + self.need, dtype=torch.int64, device=dev)))
        self._want = (lo.clone(), hi.clone())
        return self

    def check(self) -> torch.Tensor:
        """Offsets (int64, into the whole buffer: the inner block is [guard, guard + need)) of the guard bytes that changed since arm()."""
        if self._want is None:
            raise RuntimeError("check() before arm()")
        lo, hi = self._guards()
        bad_lo = torch.nonzero(lo != self._want[0]).reshape(-1)
        bad_hi = torch.nonzero(hi != self._want[1]).reshape(-1) + (self.guard + self.need)
        return torch.cat([bad_lo, bad_hi]).cpu()


def plant(obj, guarded, need: int = None, attr: str = "_ws"):
    """obj._ws = the inner block (or its first `need` bytes)."""
    ws = guarded.ws if need is None else guarded.view(need)
    setattr(obj, attr, ws)
    return ws


def assert_planted(obj, guarded, attr: str = "_ws"):
    ws = getattr(obj, attr)
    assert ws is not None and ws.data_ptr() == guarded.ws.data_ptr(), \
        f"{type(obj).__name__}.{attr} was replaced: the planted block was too small for the call, which then ran in a fresh one"
