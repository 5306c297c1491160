"""GPU: the argument contract of torch.ops.lrx.* (lightretriever_amd/torch_ops.py, csrc/lrx_torch.cpp), generic over the case table of
tests/torch_op_cases.py and parametrised by op.  Per op: the valid call gives the expected bits, twice; inputs are left alone and a mutated
argument changes only inside its documented region (a NaN canary holds the rest); every admitted view of every tensor gives the same bits; every
other view is refused or gives the result of its logical values; a wrong dtype, rank, length or device and an int32 argument out of range are
refused with a RuntimeError that names the op and the argument, the latter before anything is allocated; empty queries / stores; side stream.

Every view and every too-short tensor is cut from an allocation that covers what the op would touch if it took the tensor for a full contiguous
one, and integer parents are filled with one of the tensor's own (valid) values: a binding that lacked a check would give wrong bits or trample
a canary, never leave an allocation.  Every comparison is exact."""
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import torch_op_cases as C

pytestmark = pytest.mark.gpu
OPS = sorted(C.MAKE)
DEV = "cuda:0"
SWAP = {torch.float32: torch.int32, torch.int32: torch.float32, torch.int64: torch.float64, torch.float16: torch.bfloat16, torch.bfloat16: torch.float16,
        torch.uint8: torch.int8}
CASES = [(op, {}) for op in OPS] + [(op, kw) for op, kw in sorted(C.ALT.items())]      # every op, then the forms with the optional tensors given
IDS = [op if not kw else op + "-" + "-".join(sorted(kw)) for op, kw in CASES]
COUNTS = {}                      # op -> cases run, printed when the module is done (the summary of a run)


@pytest.fixture(scope="module", autouse=True)
def report_counts():
    yield
    print("\ncases per op:", OrderedDict(sorted(COUNTS.items())), "total", sum(COUNTS.values()))


@pytest.fixture(scope="module")
def lrx():
    from lightretriever_amd import torch_ops
    return torch_ops.load()


_built = {}


def built(op, **kw):
    key = (op, tuple(sorted(kw.items())))
    if key not in _built:
        _built[key] = C.MAKE[op](DEV, **kw)
    return _built[key]


def host(r):
    return tuple(np.asarray(t.detach().cpu().view(torch.int16).numpy() if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 else
                            t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t) for t in r)


def same(got, want):
    got, want = host(got), host(want)
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g.shape != w.shape or g.dtype != w.dtype or g.tobytes() != w.tobytes():
            return False
    return True


def run(lrx, op, b, args):
    ret = getattr(lrx, op)(*args.values())
    torch.cuda.synchronize()
    return b.canon(b.result(ret, args))


def tensors(op, args):
    return [(n, v) for n, v in args.items() if isinstance(v, torch.Tensor) and C.ANN[op][n]["kind"] == "tensor"]


def count(op, n=1):
    COUNTS[op] = COUNTS.get(op, 0) + n


def parent(shape, like):
    """An allocation for views of `like`: a NaN canary for floats, one of the tensor's own values for integers."""
    if like.is_floating_point() or like.numel() == 0:
        return C.canary(shape, like.dtype, like.device)
    return torch.full(shape, int(like.reshape(-1)[0]), dtype=like.dtype, device=like.device)


def with_arg(b, name, value, copy_from=False):
    """Fresh arguments with `name` replaced; copy_from: a mutated argument's view takes the fresh buffer's content (its canary)."""
    a = b.args()
    if copy_from:
        value.copy_(a[name])
    a[name] = value
    return a


def refused(lrx, op, args, arg=None):
    with pytest.raises(RuntimeError) as e:
        getattr(lrx, op)(*args.values())
    torch.cuda.synchronize()
    msg = str(e.value)
    assert op in msg, f"the refusal does not name the op {op}: {msg}"
    if arg is not None:
        assert re.search(rf"(?<![A-Za-z_]){re.escape(arg)}(?![A-Za-z_])", msg), f"the refusal does not name the argument {arg}: {msg}"


# ---- 1. baseline -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def baseline(lrx):
    cache = {}

    def get(op, **kw):
        key = (op, tuple(sorted(kw.items())))
        if key not in cache:
            b = built(op, **kw)
            cache[key] = run(lrx, op, b, b.args())
        return cache[key]
    return get


@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_baseline_equals_the_expectation_twice(lrx, baseline, op, kw):
    b = built(op, **kw)
    r = baseline(op, **kw)
    if op in C.EXACT and not kw:
        assert b.expect is not None, "the table promises a CPU expectation for this op"
    want = b.canon(b.expect) if b.expect is not None else b.canon(tuple(b.method(b.args())))
    assert same(r, want), (op, host(r), host(want))
    assert same(run(lrx, op, b, b.args()), r), "a second call gives other bits"
    count(op, 2)


# ---- 2. inputs are left alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_inputs_are_left_alone_and_outputs_keep_their_canary(lrx, op, kw):
    b = built(op, **kw)
    a = b.args()
    before = {n: v.clone() for n, v in tensors(op, a)}
    written = b.written(a)
    assert set(written) == {n for n in C.mutated(op) if a[n] is not None}
    run(lrx, op, b, a)
    for n, v in tensors(op, a):
        if n not in written:
            assert same((v,), (before[n],)), f"{op} changed its input {n}"
        else:
            keep = ~written[n].to(v.device).reshape(v.shape)
            assert same((v[keep],), (before[n][keep],)), f"{op} wrote {n} outside its documented region"
    count(op)


# ---- 3. admitted views -----------------------------------------------------------------------------------------------------------------------
def offset_view(t):
    """The same values at a storage offset of 32 bytes inside a larger buffer."""
    off = 32 // t.element_size()
    buf = parent((t.numel() + 2 * off,), t)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def wide_view(t, extra):
    p = parent((t.shape[0], t.shape[1] + extra), t)
    v = p[:, :t.shape[1]]
    v.copy_(t)
    return v


@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_admitted_views_give_the_same_bits(lrx, baseline, op, kw):
    b = built(op, **kw)
    r = baseline(op, **kw)
    for n, t in tensors(op, b.args()):
        ann = C.ANN[op][n]
        forms = [("offset", offset_view)]
        if ann["rows_may_stride"] and t.shape[0] > 1:
            forms += [("ld = W + 64", lambda t: wide_view(t, 64)), ("ld = W + 4", lambda t: wide_view(t, 4))]
        for what, form in forms:
            a = with_arg(b, n, form(t), copy_from=n in C.mutated(op))
            if "ld =" in what and n in C.SAME_STRIDE and isinstance(a.get(C.SAME_STRIDE[n]), torch.Tensor):
                a[C.SAME_STRIDE[n]] = form(a[C.SAME_STRIDE[n]])             # the pair shares one row stride by contract
            assert same(run(lrx, op, b, a), r), f"{op}: {n} as {what} gives other bits"
            count(op)
    if kw:
        return
    singles = []                                                             # (operand, arguments with that operand one contiguous row, their builder)
    if op in C.SINGLE_ROW:
        n, kw1 = C.SINGLE_ROW[op]
        singles.append((n, built(op, **kw1).args, built(op, **kw1)))
    for n in C.SINGLE_ROW_DERIVED.get(op, ()):
        singles.append((n, lambda n=n: C.single_row(op, b.args(), n), b))
    for n, args1, b1 in singles:                                             # a single row cut from a wider, taller parent: its stride means nothing
        r1 = run(lrx, op, b1, args1())
        a = args1()
        t = a[n]
        assert t.shape[0] == 1 and t.is_contiguous()
        p = parent((4, t.shape[1] + 64), t)
        v = p[2:3, :t.shape[1]]
        v.copy_(t)
        assert v.stride(0) != t.shape[1]
        a[n] = v
        assert same(run(lrx, op, b1, a), r1), f"{op}: a single-row {n} cut from a wider parent gives other bits"
        count(op)


# ---- 4. every other view is refused or right ---------------------------------------------------------------------------------------------------
def other_views(t, ann):
    """(name, view, logical values differ from t) for the forms the contract does not admit by name."""
    out = []
    if t.dim() == 2 and t.shape[0] > 1:
        if not ann["rows_may_stride"]:
            out.append(("strided rows", wide_view(t, 64), False))
        buf = t.t().contiguous()
        out.append((".t() of a [W, n] buffer", buf.t(), False))
        base = t.clone()
        out.append(("expand from one row", base[0:1].expand(t.shape[0], t.shape[1]), True))
    if t.dim() >= 1 and t.shape[0] > 1:
        p = parent((2 * t.shape[0],) + tuple(t.shape[1:]), t)
        v = p[::2]
        v.copy_(t)
        out.append(("[::2]", v, False))
    e = 4 // t.element_size() if t.element_size() <= 4 else 0
    if e and t.dim() == 2:
        p = parent((t.shape[0], t.shape[1] + 64), t)
        v = p[:, e:e + t.shape[1]]
        v.copy_(t)
        out.append(("a column-offset view, 4 but not 16 bytes aligned", v, False))
    elif e and t.dim() == 1 and t.numel():
        p = parent((t.numel() + 64,), t)
        v = p[e:e + t.numel()]
        v.copy_(t)
        out.append(("an offset view, 4 but not 16 bytes aligned", v, False))
    return out


@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_every_other_view_is_refused_or_right(lrx, baseline, op, kw):
    b = built(op, **kw)
    r = baseline(op, **kw)
    for n, t in tensors(op, b.args()):
        if n in C.mutated(op):
            t = b.args()[n]
        for what, v, differs in other_views(t, C.ANN[op][n]):
            assert v.data_ptr() % 4 == 0 or t.element_size() < 4
            a = b.args()
            a[n] = v
            try:
                got = run(lrx, op, b, a)
            except RuntimeError as e:
                assert op in str(e), f"{op}: {n} as {what}: the refusal does not name the op: {e}"
                count(op)
                continue
            want = r
            if differs:                                                       # right = the result for the view's logical values
                a2 = b.args()
                a2[n] = v.contiguous()
                want = run(lrx, op, b, a2)
            assert same(got, want), f"{op}: {n} as {what} was taken and gives other bits than its values do"
            count(op)


# ---- 5. wrong dtype, rank, length and device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_wrong_dtype_rank_length_and_device_are_refused(lrx, op, kw):
    b = built(op, **kw)
    base = b.args()
    n_tensors = len(tensors(op, base))
    for n, t in tensors(op, base):
        ann = C.ANN[op][n]
        bad = []
        if ann["dtype"] not in ("any", "any16"):
            assert t.dtype == C.TORCH_DTYPE[ann["dtype"]]
            bad.append(("the same bytes as " + str(SWAP[t.dtype]), t.view(SWAP[t.dtype])))
        if ann["dtype"] != "any":
            bad.append(("one dimension more", t.unsqueeze(0)))
            if t.numel():
                bad.append(("one dimension less", t.reshape(-1) if t.dim() > 1 else t[0]))
            bad.append(("a CPU tensor", t.cpu()))
        for what, v in bad:
            a = b.args()
            a[n] = v
            # (an op's only tensor on the CPU never reaches the binding: the dispatcher finds no CPU kernel and names the op alone)
            refused(lrx, op, a, n if (what != "a CPU tensor" or n_tensors > 1) else None)
            count(op)
    lengths = list(b.bad_lengths(base))
    if isinstance(base.get("q"), torch.Tensor):                               # q of another D
        lengths.append(("q", torch.zeros(base["q"].shape[0], base["q"].shape[1] + 64, device=DEV)[:, :base["q"].shape[1] + 4].contiguous()))
    for n, v in lengths:
        a = b.args()
        a[n] = v
        refused(lrx, op, a, n)
        count(op)


@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_a_tensor_on_another_device_is_refused(lrx, op, kw):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: the second-GPU cases need torch.cuda.device_count() >= 2")
    b = built(op, **kw)
    for n, t in tensors(op, b.args())[1:]:
        a = b.args()
        a[n] = t.to("cuda:1")
        refused(lrx, op, a, n)
        count(op)


# ---- 6. integers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_narrowed_integers_are_range_checked_before_any_allocation(lrx, op, kw):
    b = built(op, **kw)
    for n, ann in C.ANN[op].items():
        if ann["kind"] != "int" or not ann["int32"]:
            continue
        lo, hi = ann["range"]
        hi = b.int_hi[n] if isinstance(hi, str) else hi
        valid = b.int_valid.get(n, b.args()[n])
        assert lo <= valid <= hi
        for v in (lo - 1, hi + 1):
            a = b.args()
            a[n] = v
            refused(lrx, op, a, n)
            count(op)
        a = b.args()
        a[n] = 2 ** 32 + valid
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.max_memory_allocated()
        refused(lrx, op, a, n)
        assert torch.cuda.max_memory_allocated() - start < 1 << 20, f"{op}: {n} = 2^32 + {valid} was refused only after an allocation"
        count(op)


# ---- 7. empty ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(C.EMPTY))
def test_no_query_and_no_row_against_fp64(lrx, op):
    for kw in C.EMPTY[op]:
        b = built(op, **kw)
        assert b.expect is not None
        r = run(lrx, op, b, b.args())
        assert same(r, b.canon(b.expect)), (op, kw, host(r), host(b.expect))
        count(op)


@pytest.mark.parametrize("op", C.SEARCH_OPS)
def test_every_search_op_without_queries_and_without_rows(lrx, op):
    """Q = 0 and n_rows = 0, derived from the valid call: what every index class returns -- the shapes, (-FLT_MAX, -1), lims of zeros."""
    b = built(op)
    for what, form in (("no query", C.no_query), ("no row", C.no_row)):
        a = form(op, b.args())
        r = run(lrx, op, b, a)
        assert same(r, b.canon(C.empty_result(op, a))), (op, what, host(r))
        count(op)


# ---- 8. stream and device guard ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_side_stream_equals_the_baseline(lrx, baseline, op, kw):
    b = built(op, **kw)
    r = baseline(op, **kw)
    a = b.args()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        ret = getattr(lrx, op)(*a.values())
    s.synchronize()
    assert same(b.canon(b.result(ret, a)), r)
    count(op)


@pytest.mark.parametrize("op,kw", CASES, ids=IDS)
def test_call_while_another_device_is_current(lrx, baseline, op, kw):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: the device-guard case needs torch.cuda.device_count() >= 2")
    b = built(op, **kw)
    r = baseline(op, **kw)
    a = b.args()
    with torch.cuda.device(1):
        ret = getattr(lrx, op)(*a.values())
    torch.cuda.synchronize(DEV)
    assert same(b.canon(b.result(ret, a)), r)
    count(op)
