"""The reference of the attention kernels, written once: softmax(Q K^T / sqrt(d)) V of the fp16 inputs in float64, the error bound every
comparison with it uses, and a CPU restatement of the kernels' documented arithmetic that calibrates the bound.  Plain torch, on whichever
device the inputs are on; nothing from lightretriever_amd.

Layouts are the kernels': qkv [T, (nq + 2 nkv) d] = q heads | k heads | v heads per token row, sequences packed back to back, cu their
boundaries; q head h reads kv head h // (nq / nkv).

The bound, for every output element (O the exact result, A = P.|V| the same convex combination of the absolute values):

    |got - O| <= 2^-8 |O| + c 2^-11 A + 1e-6,    c = C_BOUND = 2

2^-8 is bf16's unit roundoff (the one rounding of the output), 2^-11 fp16's (each probability is rounded once before P.V; the row sum l
keeps the unrounded ones, so numerator and denominator differ by exactly that rounding, weighted like A), one more unit of 2^-11 for
everything done in fp32 (score accumulation over d, exp2, the running rescale, the fp32 sums over the keys), 1e-6 for probabilities that
are denormal in fp16 (spacing 2^-24 each).  Derived, not tuned: the measured ratios are in tests/test_gpu_attn_reference.py's docstring.

fp16 output (out_f16, the O-projection's operand under precise_stream = 2): the same formula with the output term at fp16's unit roundoff,

    |got - O| <= 2^-11 |O| + c 2^-11 A + 1e-6,    c = 2 unchanged

-- only the last conversion differs, so only its term does.  With the 2^-8 term gone the bound is 2.7 to 8 times tighter (A >= |O|): the
kernels' internal error, which a bf16-output comparison sees under a rounding eight times its size, is resolved.  The restatement with an
fp16 output stays inside it on every host regime (tests/test_attn_reference_host.py; figures in the GPU file's docstring)."""
import math

import torch

C_BOUND = 2.0
U_BF16 = 2.0 ** -8
U_FP16 = 2.0 ** -11
_BUDGET = 1 << 25      # fp64 score elements per chunk (256 MiB)
_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
_U_OUT = {"bf16": U_BF16, "fp16": U_FP16}


def _cu_list(cu):
    return [int(x) for x in (cu.tolist() if hasattr(cu, "tolist") else cu)]


def _heads(x, nq, nkv, d):
    """[..., (nq + 2 nkv) d] -> q [..., nkv, grp, d], k [..., nkv, d], v [..., nkv, d]"""
    lead = x.shape[:-1]
    q = x[..., :nq * d].reshape(*lead, nkv, nq // nkv, d)
    k = x[..., nq * d:(nq + nkv) * d].reshape(*lead, nkv, d)
    v = x[..., (nq + nkv) * d:].reshape(*lead, nkv, d)
    return q, k, v


def causal_gqa_fp64(qkv, cu, nq, nkv, d):
    """(O, A) float64 [T, nq d].  Sequences of equal length run as one batch, the query rows of long ones in chunks."""
    cu = _cu_list(cu)
    T, dev = qkv.shape[0], qkv.device
    grp = nq // nkv
    O = torch.zeros(T, nq * d, dtype=torch.float64, device=dev)
    A = torch.zeros_like(O)
    by_len = {}
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            by_len.setdefault(cu[b + 1] - cu[b], []).append(cu[b])
    for L, starts in by_len.items():
        rows = max(1, min(L, _BUDGET // (nq * L)))
        bc = max(1, _BUDGET // (nq * L * rows))
        ar = torch.arange(L, device=dev)
        for b0 in range(0, len(starts), bc):
            idx = torch.tensor(starts[b0:b0 + bc], device=dev)[:, None] + ar[None, :]          # [B, L] token rows
            B = idx.shape[0]
            q, k, v = _heads(qkv[idx].double(), nq, nkv, d)                                      # [B, L, nkv, ...]
            k, v = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)                                  # [B, nkv, L, d]
            for r0 in range(0, L, rows):
                r1 = min(L, r0 + rows)
                qc = q[:, r0:r1].permute(0, 2, 3, 1, 4).reshape(B, nkv, grp * (r1 - r0), d)      # rows (head in group, q row)
                s = (qc @ k[:, :, :r1].transpose(-1, -2)) * d ** -0.5
                s = s.view(B, nkv, grp, r1 - r0, r1)
                s.masked_fill_(ar[None, :r1] > ar[r0:r1, None], float("-inf"))
                p = torch.softmax(s, -1).view(B, nkv, grp * (r1 - r0), r1)
                for dst, vv in ((O, v[:, :, :r1]), (A, v[:, :, :r1].abs())):
                    o = (p @ vv).view(B, nkv, grp, r1 - r0, d).permute(0, 3, 1, 2, 4).reshape(B, r1 - r0, nq * d)
                    dst[idx[:, r0:r1]] = o
    return O, A


def prefix_suffix_fp64(suffix_qkv, prefix_kv, n, S2, nq, nkv, d):
    """(O, A) float64 [n S2, nq d]: suffix token j of a sequence attends to the P1 shared prefix keys (prefix_kv [P1, 2 nkv d] = k | v) and to
    its sequence's own suffix keys 0..j."""
    dev = suffix_qkv.device
    grp, P1 = nq // nkv, prefix_kv.shape[0]
    q, k, v = _heads(suffix_qkv.double().view(n, S2, -1), nq, nkv, d)
    pk = prefix_kv.double()[:, :nkv * d].reshape(P1, nkv, d).permute(1, 0, 2)                  # [nkv, P1, d]
    pv = prefix_kv.double()[:, nkv * d:].reshape(P1, nkv, d).permute(1, 0, 2)
    qc = q.permute(0, 2, 3, 1, 4)                                                               # [n, nkv, grp, S2, d]
    k, v = k.permute(0, 2, 1, 3)[:, :, None], v.permute(0, 2, 1, 3)[:, :, None]                 # [n, nkv, 1, S2, d]
    s_pre = qc @ pk[None, :, None].transpose(-1, -2)                                            # [n, nkv, grp, S2, P1]
    s_own = qc @ k.transpose(-1, -2)                                                            # [n, nkv, grp, S2, S2]
    ar = torch.arange(S2, device=dev)
    s_own = s_own.masked_fill(ar[None, :] > ar[:, None], float("-inf"))
    p = torch.softmax(torch.cat([s_pre, s_own], -1) * d ** -0.5, -1)
    out = []
    for f in (lambda t: t, torch.abs):
        o = p[..., :P1] @ f(pv)[None, :, None] + p[..., P1:] @ f(v)
        out.append(o.permute(0, 3, 1, 2, 4).reshape(n * S2, nq * d))
    return out[0], out[1]


def restated(qkv, cu, nq, nkv, d, lazy_t=8.0, fmt="bf16"):
    """The kernels' documented arithmetic on the CPU, bf16 [T, nq d]: fp16 q | k | v, fp32 scores, online softmax per 32-key sub-tile in the
    exp2 domain with the 1/sqrt(d) log2(e) scale folded into the exponent, a reference maximum that moves only once the row maximum has
    outgrown it by 2^lazy_t, the row sum l taken from the unrounded probabilities, P rounded to fp16 before P.V, fp32 accumulation, one
    bf16 rounding of O / l (fmt = "fp16": one fp16 rounding, the out_f16 launches).  The calibration object of the bound; it touches no
    project kernel and is not under test."""
    cu = _cu_list(cu)
    x = qkv.detach().cpu().to(torch.float16).float()
    T = x.shape[0]
    grp = nq // nkv
    c = torch.tensor((1.0 / math.sqrt(d)) * 1.4426950408889634, dtype=torch.float32)
    out = torch.zeros(T, nq * d, dtype=_DTYPE[fmt])
    for b in range(len(cu) - 1):
        s0, L = cu[b], cu[b + 1] - cu[b]
        if L <= 0:
            continue
        q, k, v = _heads(x[s0:s0 + L], nq, nkv, d)
        q = q.permute(1, 2, 0, 3)                                       # [nkv, grp, L, d]
        k, v = k.permute(1, 0, 2)[:, None], v.permute(1, 0, 2)[:, None]  # [nkv, 1, L, d]
        o = torch.zeros(nkv, grp, L, d)
        m = torch.full((nkv, grp, L), -1e30)
        l = torch.zeros(nkv, grp, L)
        row = torch.arange(L)
        for u0 in range(0, L, 32):
            u1 = min(L, u0 + 32)
            rs = slice(u0, L)                                           # rows that see this sub-tile at all
            s = q[:, :, rs] @ k[:, :, u0:u1].transpose(-1, -2)          # raw fp32 scores
            s = torch.where(torch.arange(u0, u1)[None, :] > row[rs, None], torch.tensor(-1e30), s)
            mloc = s.max(-1).values
            grow = (mloc - m[:, :, rs]) * c > lazy_t
            mnew = torch.where(grow, mloc, m[:, :, rs])
            alpha = torch.where(grow, torch.exp2((m[:, :, rs] - mnew) * c), torch.ones(()))
            p = torch.exp2(s * c + (-mnew * c)[..., None])
            l[:, :, rs] = l[:, :, rs] * alpha + p.sum(-1)
            o[:, :, rs] = o[:, :, rs] * alpha[..., None] + p.to(torch.float16).float() @ v[:, :, u0:u1]
            m[:, :, rs] = mnew
        res = o * (1.0 / l)[..., None]
        out[s0:s0 + L] = res.permute(2, 0, 1, 3).reshape(L, nq * d).to(_DTYPE[fmt])
    return out


def bound(O, A, c=C_BOUND, fmt="bf16"):
    return _U_OUT[fmt] * O.abs() + c * U_FP16 * A + 1e-6


def worst_ratio(got, O, A, c=C_BOUND, fmt="bf16"):
    """max over the elements of |got - O| / bound (nan if got holds one)"""
    r = (got.double() - O).abs() / bound(O, A, c, fmt)
    return float(r.max()) if r.numel() else 0.0


def bf16_of_fp16_allowed(h):
    """The two roundings of one number.  A launch with fp16 output and the same launch with bf16 output round the SAME fp32 value v: fp16
    keeps 11 significant bits of it, bf16 8, and fp16's grid contains bf16's wherever the fp16 value is normal, so
    bf16(v) = bf16(fp16(v)) -- unless fp16(v) is exactly the midpoint of two bf16 numbers: then v may lie on either side of it (or on it)
    and either neighbour is allowed.  h: the fp16 output.  -> (a, b, checked): the bf16 numbers the bf16 launch may hold (a == b away from
    midpoints; at one, a is the neighbour towards zero and b the one away from it), and where the statement applies (|h| >= 2^-14; below,
    fp16's spacing is no finer than bf16's).  Integer arithmetic on the fp32 bit pattern: an fp16 number is an fp32 number whose low 13
    bits are zero, a bf16 number one whose low 16 are -- no power function of the device is trusted with an exact result."""
    bits = h.float().view(torch.int32)
    rem = bits & 0xFFFF
    toward, away = (bits - rem).view(torch.float32).double(), (bits - rem + 0x10000).view(torch.float32).double()
    return torch.where(rem > 0x8000, away, toward), torch.where(rem >= 0x8000, away, toward), h.float().abs() >= 2.0 ** -14


def norm_ratio(got, O):
    """the existing tests' second check: || got || / || O || over the whole output"""
    return float(got.double().norm() / O.norm())
