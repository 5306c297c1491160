"""Row selector of the four inverted-file indexes: the faiss SearchParameters(sel=IDSelectorBatch / IDSelectorBitmap / IDSelectorRange /
IDSelectorNot) surface over the lrx_selector_* kernels (csrc/lrx_search_selector.h).

    sel = RowSelector.from_rows(rows_of_one_source, idx.ntotal)        # IDSelectorBatch
    D, I = idx.search(q, 100, sel=sel)                                 # the top 100 over the selected rows of the probed cells
    D, I = idx.search(q, 100, sel=sel.invert())                        # IDSelectorNot: a block list

A selector is a bitmap over the ORIGINAL rows 0 .. n - 1 of an index -- the number a search reports before id_base / row_map, not a stored
position and not a mapped id.  Bit r is (words[r >> 5] >> (r & 31)) & 1; `words` is a contiguous int32 CUDA tensor of ceil(n / 32) entries whose
bits at or beyond n are 0 (every constructor writes them so; the scans never read them).  Built by small HIP kernels, no torch kernel on the
way: a selector is typically made per query batch.  set_mask_ / set_rows_ rewrite the SAME storage, so a captured search replays under a new
filter."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops


class RowSelector:
    def __init__(self, n: int, device: Optional[torch.device] = None):
        """All clear."""
        if not 0 <= int(n) < (1 << 32):
            raise ValueError(f"RowSelector: n={n} out of range (0 .. 2^32 - 1)")
        _lib.require_gpu()
        self.n = int(n)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError(f"RowSelector: the words live on the GPU, not on {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.words = torch.empty((self.n + 31) // 32, dtype=torch.int32, device=self.device)
        self._fill(self.words, self.n, 0)

    # -- the four kernels, on the selector's device and the current stream -----------------------------------------------------
    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(*args, ops._s()))

    def _fill(self, words: torch.Tensor, n_bits: int, value: int):
        self._call(_lib.lib().lrx_selector_fill, _lib.ptr(words), n_bits, value)

    # -- constructors ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_mask(cls, mask, device: Optional[torch.device] = None) -> "RowSelector":
        """mask: bool [n], a torch tensor on any device or a numpy array (faiss IDSelectorBitmap)."""
        mask = torch.as_tensor(mask)
        if mask.dim() != 1:
            raise ValueError(f"RowSelector.from_mask: mask must be bool [n], got {tuple(mask.shape)}")
        return cls(mask.shape[0], device if device is not None else (mask.device if mask.is_cuda else None)).set_mask_(mask)

    @classmethod
    def from_rows(cls, rows, n: int, device: Optional[torch.device] = None) -> "RowSelector":
        """rows: int64 row numbers, duplicates are fine (faiss IDSelectorBatch).  A row outside [0, n) is skipped and counted in
        lrx_device_error_count."""
        rows = torch.as_tensor(rows)
        return cls(n, device if device is not None else (rows.device if rows.is_cuda else None)).set_rows_(rows)

    @classmethod
    def from_range(cls, lo: int, hi: int, n: int, device: Optional[torch.device] = None) -> "RowSelector":
        """Rows [lo, hi) (faiss IDSelectorRange), clamped to [0, n)."""
        sel = cls(n, device)
        lo, hi = max(int(lo), 0), min(int(hi), sel.n)
        if lo < hi:
            # [lo, hi) = NOT [0, lo) below hi: a scratch bitmap of hi bits with its first lo set, inverted into the first words of the selector
            # (which is clear beyond them) -- the four kernels, no fifth
            tmp = torch.empty((hi + 31) // 32, dtype=torch.int32, device=sel.device)
            sel._fill(tmp, hi, 0)
            sel._fill(tmp, lo, 1)
            sel._call(_lib.lib().lrx_selector_invert, _lib.ptr(tmp), _lib.ptr(sel.words), hi)
        return sel

    # -- in place: the same `words` storage ----------------------------------------------------------------------------------------------
    def set_mask_(self, mask) -> "RowSelector":
        mask = torch.as_tensor(mask)
        if mask.dtype != torch.bool or tuple(mask.shape) != (self.n,):
            raise ValueError(f"RowSelector.set_mask_: mask must be bool [{self.n}], got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.to(self.device).contiguous()
        self._call(_lib.lib().lrx_selector_from_mask, _lib.ptr(mask), self.n, _lib.ptr(self.words))
        return self

    def set_rows_(self, rows) -> "RowSelector":
        """Exactly the given rows: the bitmap is cleared first."""
        rows = torch.as_tensor(rows)
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise ValueError(f"RowSelector.set_rows_: rows must be int64 [m], got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.to(self.device).contiguous()
        self._fill(self.words, self.n, 0)
        self._call(_lib.lib().lrx_selector_set_rows, _lib.ptr(rows), rows.shape[0], self.n, _lib.ptr(self.words))
        return self

    # -- derived ----------------------------------------------------------------------------------------------------------------------
    def invert(self) -> "RowSelector":
        """A new selector of the rows this one leaves out (faiss IDSelectorNot); its tail bits are clear."""
        out = RowSelector(self.n, self.device)
        self._call(_lib.lib().lrx_selector_invert, _lib.ptr(self.words), _lib.ptr(out.words), self.n)
        return out

    def to_mask(self) -> torch.Tensor:
        """bool CUDA [n]."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.device)
        return (((self.words[:, None] >> shifts) & 1) != 0).reshape(-1)[:self.n]

    def count(self) -> int:
        """The number of selected rows (reads back to the host)."""
        return int(self.to_mask().sum().item())

    def __repr__(self):
        return f"RowSelector(n={self.n}, device={self.device})"


def check_selector(sel, ntotal: int, device: torch.device, who: str) -> Optional[torch.Tensor]:
    """The checks a search makes of its `sel` argument -> the words to hand to the library (None: no selector)."""
    if sel is None:
        return None
    if not isinstance(sel, RowSelector):
        raise TypeError(f"{who}: sel must be a RowSelector, got {type(sel).__name__}")
    if sel.n != ntotal:
        raise ValueError(f"{who}: the selector covers {sel.n} rows but the index holds {ntotal} (make it after the last add())")
    if sel.words.device != torch.device(device):
        raise ValueError(f"{who}: the selector is on {sel.words.device}, the index on {device}")
    return sel.words
