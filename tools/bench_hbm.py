"""Practical HBM read ceiling on this box: time simple streaming reads of an 8 GB fp32 buffer with library kernels.
Importable: legs() returns {leg: (ms, GB/s)}, ceiling() the best read leg (what the other bench tools quote as the stream-read ceiling)."""
import torch


def t(fn, n=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def legs(rows=1_000_000, cols=2048):
    x = torch.randn(rows, cols, device="cuda")
    B = x.numel() * 4
    out = {}
    for name, fn in [("sum", lambda: x.sum()), ("abs().max", lambda: x.abs().max()), ("sum(dim=1)", lambda: x.sum(dim=1)), ("sum(dim=0)", lambda: x.sum(dim=0)),
                     ("matvec fp32", lambda: x @ x[0]), ("copy (r+w)", lambda: x.clone())]:
        ms = t(fn)
        out[name] = (ms, B / ms / 1e6 * (2 if 'copy' in name else 1))
    return out


def ceiling(rows=1_000_000, cols=2048):
    """(leg, GB/s) of the fastest pure-read leg."""
    name, (ms, gbps) = max(((n, v) for n, v in legs(rows, cols).items() if "copy" not in n), key=lambda kv: kv[1][1])
    return name, gbps


if __name__ == "__main__":
    for name, (ms, gbps) in legs().items():
        print(f"{name:14s} {ms:.3f} ms  {gbps:.0f} GB/s")
