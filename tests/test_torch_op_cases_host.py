"""CPU: the case table of the torch-op contract tests (tests/torch_op_cases.py) against the registration itself -- the names of
TORCH_LIBRARY(lrx, ...), torch_ops.OPS and the table are one set, every schema argument carries exactly one annotation of the right kind,
the schema's (a!) marks are the table's mutated arguments -- and the CPU-computed expectations against themselves."""
import os
import re

import numpy as np
import pytest
import torch

import torch_op_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "lightretriever_amd", "csrc", "lrx_torch.cpp")


@pytest.fixture(scope="module")
def lrx():
    from lightretriever_amd import torch_ops
    return torch_ops.load()


def registered():
    src = open(SRC).read()
    return re.findall(r'm\.def\("(\w+)\(', src), re.findall(r'm\.impl\("(\w+)"', src)


def test_registration_ops_list_and_table_are_one_set(lrx):
    from lightretriever_amd import torch_ops
    defs, impls = registered()
    assert len(defs) == len(set(defs)) == 41 and sorted(defs) == sorted(impls)
    assert set(defs) == set(torch_ops.OPS) == set(C.ANN) and len(torch_ops.OPS) == len(defs)
    assert set(C.MAKE) == set(C.ANN) and set(C.EXACT) <= set(C.MAKE) and set(C.EMPTY) <= set(C.MAKE) and set(C.SINGLE_ROW) <= set(C.MAKE)
    assert set(C.ALT) <= set(C.MAKE) and len(C.SEARCH_OPS) == 30 and set(C.EMPTY) - {"linear_transform"} <= set(C.SEARCH_OPS)
    # every rows-may-stride operand of every op has a single-row case, from its builder or derived from the valid call
    for op in C.ANN:
        have = set(C.SINGLE_ROW_DERIVED.get(op, ())) | ({C.SINGLE_ROW[op][0]} if op in C.SINGLE_ROW else set())
        assert have == {a for a, n in C.ANN[op].items() if n["kind"] == "tensor" and n["rows_may_stride"]}, op
    assert sum(name.startswith("ivf_") for name in defs) == 16


@pytest.mark.parametrize("op", sorted(C.ANN))
def test_every_schema_argument_is_annotated(lrx, op):
    schema = getattr(lrx, op).default._schema
    names = [a.name for a in schema.arguments]
    assert names == list(C.ANN[op]), "the table lists the schema's arguments, in the schema's order"
    for a in schema.arguments:
        ann, ty = C.ANN[op][a.name], str(a.type)
        want = {"Tensor": "tensor", "Optional[Tensor]": "tensor", "int": "int", "float": "float", "bool": "bool"}[ty]
        assert ann["kind"] == want, (a.name, ty, ann)
        if want == "tensor":
            assert ann["optional"] == (ty == "Optional[Tensor]"), a.name
            assert ann["dtype"] in C.TORCH_DTYPE or ann["dtype"] in ("any16", "any")
            assert not ann["rows_may_stride"] or ann["rank"] == 2
        if want == "int" and ann["int32"]:
            lo, hi = ann["range"]
            assert isinstance(lo, int) and (isinstance(hi, str) or lo <= hi <= C.I32_MAX)


@pytest.mark.parametrize("op", sorted(C.ANN))
def test_schema_write_marks_equal_the_mutated_set(lrx, op):
    schema = getattr(lrx, op).default._schema
    marked = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert marked == C.mutated(op)
    assert all(r.alias_info is None for r in schema.returns)


def test_rows_may_stride_is_what_the_contract_names():
    from lightretriever_amd import torch_ops
    table = {a for op in C.ANN for a, n in C.ANN[op].items() if n["kind"] == "tensor" and n["rows_may_stride"]}
    assert table == set(torch_ops.ROWS_MAY_STRIDE)
    assert all(re.search(rf"\b{a}\b", torch_ops.__doc__) for a in torch_ops.ROWS_MAY_STRIDE)


def test_fp64_references_check_themselves():
    X, q = C._flat_data()
    Dd, I, R = C.topk_fp64(q, X, C.K, 11)
    assert Dd.shape == I.shape == (C.Q, C.K) and Dd.dtype == np.float32 and I.dtype == np.int64
    assert ((I >= 11) & (I < 11 + C.N)).all() and (np.diff(Dd.astype(np.float64), axis=1) <= 0).all() and (I - 11 == R).all()
    S = q.astype(np.float64) @ X.astype(np.float64).T
    assert (S == S.astype(np.float32)).all(), "grid scores are exact in fp32"
    for i in range(C.Q):
        assert (Dd[i] == S[i, R[i]]).all() and (S[i] > Dd[i, -1]).sum() <= C.K - 1
        ties = Dd[i, :-1] == Dd[i, 1:]
        assert (R[i, :-1][ties] < R[i, 1:][ties]).all()                       # ties to the lower row
    Dp, Ip, _ = C.topk_fp64(q, X[:3], C.K)                                   # past the rows: (-FLT_MAX, -1)
    assert (Ip[:, 3:] == -1).all() and (Dp[:, 3:] == -C.FLT_MAX).all() and (Ip[:, :3] >= 0).all()
    assert C.topk_fp64(q[:0], X, C.K)[0].shape == (0, C.K) and (C.topk_fp64(q, X[:0], C.K)[1] == -1).all()
    lims, Dr, Ir = C.range_fp64(q, X, 0.03125, 5)
    assert lims[0] == 0 and lims[-1] == Dr.size == Ir.size and (np.diff(lims) > 0).all() and (np.diff(lims) < C.N).all()
    assert (Dr > 0.03125).all() and ((Ir >= 5) & (Ir < 5 + C.N)).all()
    for a, b in zip(lims[:-1], lims[1:]):
        assert (np.diff(Ir[a:b]) > 0).all()
    assert int((S.astype(np.float32) > np.float32(0.03125)).sum()) == lims[-1]
    assert C.range_fp64(q[:0], X, 0.0)[0].tolist() == [0] and C.range_fp64(q, X[:0], 0.0)[0].tolist() == [0] * (C.Q + 1)


def test_merge_pack_and_tile_references_check_themselves():
    d, i = C._parts()
    Dm, Im = C.merge_fp64(d, i)
    assert Dm.shape == (C.Q, C.K) and (np.diff(Dm.astype(np.float64), axis=1) <= 0).all() and (Im >= 0).all()
    for qi in range(C.Q):
        assert Dm[qi, 0] == d[:, qi].max() and set(Im[qi]) <= set(i[:, qi].reshape(-1))
    w = C.pack_words(d, i)
    assert ((w >> 32).astype(np.int32).view(np.float32).reshape(d.shape) == d).all() and ((w & 0xFFFFFFFF)[i >= 0] == i[i >= 0]).all()
    assert ((w & 0xFFFFFFFF)[i < 0] == 0xFFFFFFFF).all()
    # the tiling is the inverse of _TiledIPIndex.shadow_rows' view
    X16 = (np.arange(130 * 64).reshape(130, 64) % 2039).astype(np.float16)
    tiled, mask = C.tile_shadow(X16, 2, row0=40)
    back = lambda a: torch.from_numpy(a).view(2, 1, 8, 2, 4, 16, 8).permute(0, 2, 5, 1, 3, 4, 6).reshape(256, 64).numpy()
    assert (back(tiled)[40:170] == X16).all() and back(mask)[40:170].all() and mask.sum() == 130 * 64 and not back(tiled)[:40].any()
    b = C.bounds_fp64(C._flat_data()[0])
    assert b.dtype == np.float32 and b[0] > 0 and b[1] == 0                     # grid rows are exact in fp16


def test_grid_values_are_exact_in_every_format():
    g = C.grid(np.random.default_rng(0), (50, 64))
    t = torch.from_numpy(g)
    assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t) and (np.abs(g) <= 0.125).all() and ((g * 64) % 1 == 0).all()
