"""SparseRows: quantised sparse vectors as a ragged CSR that stays where it was made -- what ops.sparse_compact_csr produces on the GPU and
ImpactSearch.index / retrieve_with_emb take without a Python object per posting.

Row i holds the (term, weight) pairs terms[row_off[i]:row_off[i + 1]] / weights[...]: a term is a token id in [0, vocab_size), in ascending order
inside a row, a weight an integer >= 1.  An empty vector is the single pair (vocab_size, 1): the device form of the reference's {"-1": 1}
(finetune/sparse_converter_mixin.py), an ordinary term.  `identity_term` is the same rule for the string terms of host-side queries."""
from __future__ import annotations

from typing import Optional

import torch

MARKER = "-1"   # the reference's term of an empty vector


def identity_term(term: str, vocab_size: int) -> Optional[int]:
    """The identity numbering of ImpactSearch for a string term: the canonical decimal form of a token id in [0, vocab_size) is that integer,
    "-1" is vocab_size (the empty-vector marker), anything else None (dropped).  Only the canonical form counts -- "007", "+7", " 7" and "7.0"
    are NOT term 7: the terms are strings to the dict numbering and to Lucene, where "007" is a term no document holds, and both numberings
    must give the same hits."""
    if term == MARKER:
        return vocab_size
    if not (term.isascii() and term.isdigit()) or (len(term) > 1 and term[0] == "0"):
        return None
    t = int(term)
    return t if t < vocab_size else None


class SparseRows:
    """row_off int64 [n + 1], terms int32 [nnz], weights int32 [nnz] on one device, vocab_size.  len() = n rows; rows[a:b] = a row range
    (reads two offsets back when the arrays are on the GPU); SparseRows.cat(parts) appends on the device; to_dicts() is the host form."""

    def __init__(self, row_off: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor, vocab_size: int):
        if row_off.dtype != torch.int64 or terms.dtype != torch.int32 or weights.dtype != torch.int32:
            raise ValueError(f"SparseRows: row_off int64, terms / weights int32 (got {row_off.dtype}, {terms.dtype}, {weights.dtype})")
        if row_off.dim() != 1 or row_off.numel() < 1 or terms.dim() != 1 or terms.shape != weights.shape:
            raise ValueError("SparseRows: row_off [n + 1], terms / weights [nnz] of one length")
        if not (row_off.device == terms.device == weights.device):
            raise ValueError("SparseRows: the three arrays live on one device")
        if int(vocab_size) < 1:
            raise ValueError(f"SparseRows: vocab_size={vocab_size}")
        self.row_off, self.terms, self.weights, self.vocab_size = row_off, terms, weights, int(vocab_size)

    def __len__(self) -> int:
        return self.row_off.numel() - 1

    @property
    def device(self) -> torch.device:
        return self.row_off.device

    @property
    def nnz(self) -> int:
        return self.terms.numel()

    def to(self, device) -> "SparseRows":
        return SparseRows(self.row_off.to(device), self.terms.to(device), self.weights.to(device), self.vocab_size)

    def __getitem__(self, rows) -> "SparseRows":
        if not isinstance(rows, slice):
            raise TypeError("SparseRows[a:b]: a row range")
        a, b, step = rows.indices(len(self))
        if step != 1:
            raise ValueError("SparseRows[a:b]: step 1 only")
        b = max(a, b)
        lo, hi = (int(x) for x in self.row_off[[a, b]].tolist())
        return SparseRows(self.row_off[a:b + 1] - lo, self.terms[lo:hi], self.weights[lo:hi], self.vocab_size)

    @classmethod
    def cat(cls, parts) -> "SparseRows":
        """The rows of `parts` in order (one vocab_size, one device); nothing leaves the device."""
        parts = list(parts)
        if not parts:
            raise ValueError("SparseRows.cat: nothing to concatenate")
        if len(parts) == 1:
            return parts[0]
        if len({p.vocab_size for p in parts}) != 1:
            raise ValueError(f"SparseRows.cat: vocab sizes differ ({sorted({p.vocab_size for p in parts})})")
        # part j's offsets are shifted by the postings before it: nnz is a shape, so no offset is read back
        offs, base = [parts[0].row_off], parts[0].nnz
        for p in parts[1:]:
            offs.append(p.row_off[1:] + base)
            base += p.nnz
        return cls(torch.cat(offs), torch.cat([p.terms for p in parts]), torch.cat([p.weights for p in parts]), parts[0].vocab_size)

    def to_dicts(self) -> list:
        """[{str(token id): weight}] per row, the marker as {"-1": ...}: what LrxHybridModel.convert_sparse_reps_to_json returns for the same
        vectors.  One copy of the three arrays to the host."""
        off = self.row_off.cpu().tolist()
        V = self.vocab_size
        names = [MARKER if t == V else str(t) for t in self.terms.cpu().tolist()]
        w = self.weights.cpu().tolist()
        return [dict(zip(names[off[i]:off[i + 1]], w[off[i]:off[i + 1]])) for i in range(len(off) - 1)]
