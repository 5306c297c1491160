"""The hand-made cells of the inverted-file GPU tests (test_gpu_ivf_range.py, test_gpu_ivf_plan_scale.py): `Store`, one family's cells under
data for which the family's numpy yardstick gives the library's bits, its three ways into the range search (the C entry, the torch op,
ops.py), and the bit comparisons the tests share.  A helper module: it holds no tests."""
import numpy as np
import torch

import ivf_range_yardstick as R
import ivf_yardstick as IV
import ivfpq_yardstick as YPQ
import ivfsq8_yardstick as YS8
import ivfsq_yardstick as YSQ

F32 = np.float32
FAMILIES = ("flat", "sq_fp16", "sq8", "pq")
SEARCH = {"flat": IV.search, "sq_fp16": YSQ.search, "sq8": YS8.search, "pq": YPQ.search}
M_PQ = 8
FILL_D, FILL_I, FILL_L = 7.5, -7, -5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def errors(reset=True):
    from lightretriever_amd import _lib
    torch.cuda.synchronize()
    return int(_lib.lib().lrx_device_error_count(1 if reset else 0))


def quarters(rng, shape):
    return (rng.integers(-12, 13, shape) / 4.0).astype(F32)


def host(t):
    return tuple(x.cpu().numpy() for x in t)


def same(got, want):
    """(lims, D, I) against (lims, D, I), tensors or arrays: bits."""
    got = host(got) if isinstance(got[0], torch.Tensor) else got
    want = host(want) if isinstance(want[0], torch.Tensor) else want
    return (np.array_equal(got[0], want[0]) and got[1].shape == want[1].shape and np.array_equal(got[1].view(np.int32), want[1].view(np.int32)) and
            np.array_equal(got[2], want[2]))


def partial(lims, scanned):
    """The yardstick's check that the result is neither empty nor everything scanned (lims: an array or a device tensor)."""
    return R.some_query_is_partial(lims.cpu().numpy() if isinstance(lims, torch.Tensor) else lims, scanned)


def slices(res, i):
    lims, D, I = res
    a, b = int(lims[i]), int(lims[i + 1])
    return D[a:b], I[a:b]


def same_slice(a, i, b, j):
    (da, ia), (db, ib) = slices(a, i), slices(b, j)
    return torch.equal(ia, ib) and torch.equal(da.view(torch.int32), db.view(torch.int32))


class Store:
    """Hand-made cells of one family: rows / codes by stored position (host and device), a non-identity row_ids, integer centroids.  Data under
    which the family's yardstick gives the library's bits: integers for the flat and fp16 stores, grid codes and quarters for the 8-bit
    store, the yardstick's own table sums for PQ."""

    def __init__(self, fam, sizes, d=64, Q=6, seed=0, by_residual=True):
        rng = np.random.default_rng(seed + 17 * FAMILIES.index(fam))
        self.fam, self.d, self.sizes, self.nlist, self.n, self.rng = fam, d, list(sizes), len(sizes), int(sum(sizes)), rng
        self.cells = rng.permutation(np.repeat(np.arange(self.nlist), sizes))
        self.row_ids, self.list_off = IV.cell_order(self.cells, self.nlist)
        assert not np.array_equal(self.row_ids, np.arange(self.n))
        self.cent = rng.integers(-3, 4, (self.nlist, d)).astype(F32)
        self.by_residual = None if fam == "flat" else bool(by_residual)
        cs = self.cells[self.row_ids]
        if fam == "flat":
            self.x = rng.integers(-3, 4, (self.n, d)).astype(F32)                          # by ORIGINAL row
            self.q = rng.integers(-3, 4, (Q, d)).astype(F32)
            stored = self.x[self.row_ids]
            self.head, self.dhead = (stored,), (dev(stored),)
        elif fam == "sq_fp16":
            self.x = rng.integers(-3, 4, (self.n, d)).astype(F32)
            self.q = rng.integers(-3, 4, (Q, d)).astype(F32)
            codes = YSQ.encode(self.x[self.row_ids], self.cent, cs) if by_residual else YSQ.encode(self.x[self.row_ids])
            self.head, self.dhead = (codes,), (dev(codes),)
        elif fam == "sq8":
            r = np.array(YS8.GRID_RANGES, np.float64)[rng.integers(0, 3, d)]
            self.trained = np.concatenate([r[:, 0], r[:, 1]]).astype(F32)
            self.q = quarters(rng, (Q, d))
            codes = rng.integers(0, 256, (self.n, d)).astype(np.uint8)
            self.head, self.dhead = (codes, self.trained), (dev(codes), dev(self.trained))
        else:
            from lightretriever_amd import PQIndex
            self.C = rng.standard_normal((M_PQ, 256, d // M_PQ)).astype(F32)
            self.q = rng.standard_normal((Q, d)).astype(F32)
            codes = rng.integers(0, 256, (self.n, M_PQ)).astype(np.uint8)
            self.head = (self.C, codes)
            self.dhead = (PQIndex(d, M_PQ).rows_to_blocked(torch.from_numpy(codes)), dev(self.C))
        self.doff, self.dids = dev(self.list_off), dev(self.row_ids)

    def base(self, shape):
        """Probe scores for hand-given probes (None for the flat family and without residuals)."""
        if not self.by_residual:
            return None
        return (3 * self.rng.standard_normal(shape)).astype(F32) if self.fam == "pq" else quarters(self.rng, shape)

    def want(self, probes, base, radius, q=None, **kw):
        q = self.q if q is None else q
        if self.fam == "flat":
            return R.expected(IV.search, (q,) + self.head, probes, self.list_off, self.row_ids, radius, **kw)
        return R.expected(SEARCH[self.fam], (q,) + self.head, probes, self.list_off, self.row_ids, radius, probe_scores=base, by_residual=self.by_residual, **kw)

    def median(self, probes, base, q=None):
        """The median score over every scanned (query, row) pair, from the yardstick."""
        return float(np.median(self.want(probes, base, -np.inf, q=q)[1]))

    # -- the three ways into the library ------------------------------------------------------------------------------------------
    def c(self, probes, base, radius, max_scan=None, capacity=None, q=None, id_base=0, row_map=None, null_out=False, fill=torch.empty):
        """The C entry through ctypes with ld_probe = nprobe + 3 (padding entries name cell 0 and carry a score of 1e30: read, they would add
        that cell's rows or lift a score) -> (lims, D, I) as written over their fill patterns, untrimmed, and the capacity used.  fill: what
        allocates the workspace (torch.zeros: a word the scan never wrote is then the null word, a missing row, not an earlier call's hit)."""
        from lightretriever_amd import _lib
        l = _lib.lib()
        q = dev(self.q if q is None else q)
        probes = np.asarray(probes, np.int64)
        Q, npb = probes.shape
        scan = self.n if max_scan is None else max_scan
        capacity = Q * self.n if capacity is None else capacity
        pb = torch.zeros(Q, npb + 3, dtype=torch.int64, device="cuda")
        pb[:, :npb] = dev(probes)
        ps = None
        if base is not None:
            ps = torch.full((Q, npb + 3), 1e30, dtype=torch.float32, device="cuda")
            ps[:, :npb] = dev(np.asarray(base, F32))
        lims = torch.full((Q + 1,), FILL_L, dtype=torch.int64, device="cuda")
        D = torch.full((max(capacity, 1),), FILL_D, dtype=torch.float32, device="cuda")
        I = torch.full((max(capacity, 1),), FILL_I, dtype=torch.int64, device="cuda")
        p = _lib.ptr
        wsa = (self.n, self.nlist, self.d) + ((M_PQ,) if self.fam == "pq" else ()) + (Q, npb, scan)
        ws = fill(getattr(l, f"lrx_ivf_{self.fam}_ip_range_workspace_bytes")(*wsa), dtype=torch.uint8, device="cuda")
        tail = (scan, float(radius), id_base, p(lims), None if null_out else p(D), None if null_out else p(I), capacity, p(row_map), p(ws), ws.numel(),
                _lib.current_stream())
        mid = (p(self.doff), p(self.dids), self.nlist, p(q), Q, p(pb))
        coded = (p(ps), npb, npb + 3, int(bool(self.by_residual)))
        if self.fam == "flat":
            xb = torch.full((self.n, self.d + 8), 1e30, dtype=torch.float32, device="cuda")     # ldx = d + 8: the padding columns are never read
            xb[:, :self.d] = self.dhead[0]
            rc = l.lrx_ivf_flat_ip_range_search(p(xb), self.n, self.d + 8, self.d, *mid, npb, npb + 3, *tail)
        elif self.fam == "sq_fp16":
            rc = l.lrx_ivf_sq_fp16_ip_range_search(p(self.dhead[0]), self.n, self.d, *mid, *coded, *tail)
        elif self.fam == "sq8":
            rc = l.lrx_ivf_sq8_ip_range_search(p(self.dhead[0]), self.n, self.d, p(self.dhead[1]), 0, *mid, *coded, *tail)
        else:
            rc = l.lrx_ivf_pq_ip_range_search(p(self.dhead[0]), self.n, p(self.dhead[1]), self.d, M_PQ, *mid, *coded, *tail)
        _lib.check(rc)
        torch.cuda.synchronize()
        return lims, D, I

    def c_trim(self, *a, **kw):
        lims, D, I = self.c(*a, **kw)
        n = int(lims[-1])
        assert (D[n:] == FILL_D).all() and (I[n:] == FILL_I).all()            # nothing written past the result
        return lims, D[:n], I[:n]

    def _op_args(self, probes, base, radius, max_scan, q, id_base, row_map):
        q = dev(self.q if q is None else q)
        probes = dev(np.asarray(probes, np.int64))
        scan = self.n if max_scan is None else max_scan
        base = None if base is None else dev(np.asarray(base, F32))
        tail = (float(radius), scan, id_base, row_map)
        if self.fam == "flat":
            return (q, self.dhead[0], self.doff, self.dids, probes) + tail
        mid = (self.doff, self.dids, probes, base, bool(self.by_residual))
        if self.fam == "sq8":
            return (q, self.dhead[0], self.dhead[1], 0) + mid + tail
        return (q,) + self.dhead + mid + tail

    def op(self, probes, base, radius, max_scan=None, q=None, id_base=0, row_map=None):
        from lightretriever_amd import torch_ops
        torch_ops.load()
        return getattr(torch.ops.lrx, f"ivf_{self.fam}_ip_range_search")(*self._op_args(probes, base, radius, max_scan, q, id_base, row_map))

    def ops(self, probes, base, radius, max_scan=None, q=None, id_base=0, row_map=None):
        from lightretriever_amd import ops
        return getattr(ops, f"ivf_{self.fam}_ip_range_search")(*self._op_args(probes, base, radius, max_scan, q, id_base, row_map))

    def all(self, probes, base, radius, **kw):
        """The C call, the torch op and ops.py, each against the yardstick -> (the C call's result, the yardstick's)."""
        want = self.want(probes, base, radius, **{k: v for k, v in kw.items() if k in ("q", "id_base")},
                         row_map=None if kw.get("row_map") is None else kw["row_map"].cpu().numpy(), max_scan_rows=kw.get("max_scan"))
        got = self.c_trim(probes, base, radius, **kw)
        assert same(got, want)
        assert same(self.op(probes, base, radius, **kw), want)
        assert same(self.ops(probes, base, radius, **kw), want)
        return got, want

    def index(self, nprobe, **kw):
        """The family's index class over these cells."""
        import lightretriever_amd as A
        if self.fam == "flat":
            idx = A.IVFFlatIndex(self.d, self.nlist, nprobe=nprobe, **kw)
            idx.set_contents(self.cent, self.head[0], self.list_off, self.row_ids)
        elif self.fam == "sq_fp16":
            idx = A.IVFSQIndex(self.d, self.nlist, nprobe=nprobe, by_residual=self.by_residual, **kw)
            idx.set_contents(self.cent, self.head[0], self.list_off, self.row_ids)
        elif self.fam == "sq8":
            idx = A.IVFSQ8Index(self.d, self.nlist, "QT_8bit", nprobe=nprobe, by_residual=self.by_residual, **kw)
            idx.set_contents(self.cent, self.trained, torch.from_numpy(self.head[0]), self.list_off, self.row_ids)
        else:
            idx = A.IVFPQIndex(self.d, self.nlist, M_PQ, nprobe=nprobe, by_residual=self.by_residual, **kw)
            idx.set_contents(self.cent, self.C, self.head[1], self.list_off, self.row_ids)
        return idx
