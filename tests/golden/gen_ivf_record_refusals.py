"""Generator of ivf_record_refusals.json: what the writers and readers of the four inverted-file records ('IwFl', 'IwPQ', 'IwSq' with an fp16
and with an 8-bit quantiser) produce, return and refuse, recorded from the commit BEFORE their shared reader / writer paths were written
(tests/test_ivf_records_host.py re-derives the same cases with the code at hand and compares).  Only public names of index_io are used, so
the script runs at either commit:

    python tests/golden/gen_ivf_record_refusals.py          # rewrites tests/golden/ivf_record_refusals.json

Records: d = 4, nlist = 3, cell sizes [2, 0, 1], nprobe = 2; PQ with M = 2; the 8-bit record with qtype 0 and 2; by_residual both ways for
the three code families.  Per record: the sha256 of the file (plain, behind a prefix, with the sizes [0, 0, 3] -- the 'sprs' form --,
untrained with sizes [0, 0], and nlist = 5 with sizes [1, 0, 2, 0, 0]: 'sprs' with two cells), the sha256 of a canonical dump of what the
reader returns, every truncation (by cutting the file, and by an `end` inside a longer file for the records that take one; inside the bulk
float arrays only the first, one middle and the last byte) and a list of single-field overwrites; the truncations and overwrites go to the
by_residual = 1 records (the flag is one byte handed through).  Every damaged file is also given to index_record_end and, 'IwSq', to
ivf_sq_qtype, whose answers are recorded the same way.  Last, writer calls with wrong arguments, some wrong in two ways.

Run it from a checkout (or a `git worktree`) of the commit whose behaviour is the yardstick, and copy the JSON over.

An outcome is "ok <value>" or "<exception type>: <text>" with the file's path replaced by <FILE>; in a truncation the cut length, where the
text quotes it as "bytes=<n>)", is replaced by <CUT> (the case names the length, so nothing is lost).  Outcomes are stored grouped by text:
text -> {"<record> <variant> <call>": items}, the items of a truncation group packed into ranges ("0-89,98")."""
import hashlib
import json
import os
import struct
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ivf_record_refusals.json")
D, M, NPROBE, PREFIX = 4, 2, 2, b"0123456"
SIZES = dict(plain=[2, 0, 1], sprs=[0, 0, 3], untrained=[0, 0], sprs2=[1, 0, 2, 0, 0])


def _arrays(sizes, trained):
    nlist, n = len(sizes), int(sum(sizes))
    cent = (np.arange(nlist * D, dtype=np.float32).reshape(nlist, D) / 8 - 1) if trained else np.zeros((0, D), np.float32)
    ids = (np.arange(n, dtype=np.int64) * 7 + 2) % 11
    return cent, ids, n


def records(io):
    """-> {name: dict(fourcc, write(fname, sizes, trained, **kw), read(fname, offset, end), takes_offset, middle: bytes between the direct map and
    'ilar', bulk: [(start, stop)] of the bulk float arrays after the centroids, relative to the end of the direct map)}."""
    out = {}

    def flat_write(f, sizes, trained=True, **kw):
        cent, ids, n = _arrays(sizes, trained)
        io.write_ivf_flat(f, cent, sizes, np.arange(n * D, dtype=np.float32).reshape(n, D) / 4 - 2, ids, nprobe=NPROBE, is_trained=trained, **kw)
    out["flat"] = dict(fourcc=b"IwFl", write=flat_write, read=lambda f, off=0, end=None: io.read_ivf_flat(f), takes_offset=False, middle=0, bulk=[])

    pqc = ((np.arange(M * 256 * (D // M)) % 97).astype(np.float32) / 16).reshape(M, 256, D // M)
    for r in (0, 1):
        def pq_write(f, sizes, trained=True, r=r, **kw):
            cent, ids, n = _arrays(sizes, trained)
            io.write_ivf_pq(f, cent, pqc, sizes, (np.arange(n * M) * 37 % 256).astype(np.uint8).reshape(n, M), ids, nprobe=NPROBE, by_residual=bool(r),
                            is_trained=trained, **kw)
        out[f"pq_r{r}"] = dict(fourcc=b"IwPQ", write=pq_write, read=io.read_ivf_pq, takes_offset=True, middle=9 + 24 + 8 + 4 * 256 * D,
                               bulk=[(9 + 24 + 8, 9 + 24 + 8 + 4 * 256 * D)])

        def sq_write(f, sizes, trained=True, r=r, **kw):
            cent, ids, n = _arrays(sizes, trained)
            io.write_ivf_sq(f, cent, sizes, (np.arange(n * D) / 4 - 1).astype(np.float16).reshape(n, D), ids, nprobe=NPROBE, by_residual=bool(r),
                            is_trained=trained, **kw)
        out[f"sq_r{r}"] = dict(fourcc=b"IwSq", write=sq_write, read=io.read_ivf_sq, takes_offset=True, middle=28 + 8 + 9, bulk=[])

        for q in (0, 2):
            n_t = 2 * D if q == 0 else 2

            def sq8_write(f, sizes, trained=True, r=r, q=q, n_t=n_t, **kw):
                cent, ids, n = _arrays(sizes, trained)
                io.write_ivf_sq8(f, cent, np.arange(n_t, dtype=np.float32) / 2 + 0.25, q, sizes, (np.arange(n * D) * 29 % 256).astype(np.uint8).reshape(n, D),
                                 ids, nprobe=NPROBE, by_residual=bool(r), is_trained=trained, **kw)
            out[f"sq8_q{q}_r{r}"] = dict(fourcc=b"IwSq", write=sq8_write, read=io.read_ivf_sq8, takes_offset=True, middle=28 + 8 + 4 * n_t + 9,
                                         bulk=[(28 + 8, 28 + 8 + 4 * n_t)])
    return out


def dump(v) -> str:
    """A canonical text of what a reader returned: keys sorted; arrays by dtype, shape and bytes."""
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {dump(v[k])}" for k in sorted(v)) + "}"
    if isinstance(v, np.ndarray):
        return f"array({v.dtype.str}, {v.shape}, {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()})"
    return f"{type(v).__name__}({v!r})"


def outcome(fn, fname, cut=None) -> str:
    try:
        v = fn()
        return "ok " + (hashlib.sha256(dump(v).encode()).hexdigest() if isinstance(v, dict) else dump(v))
    except Exception as e:                       # (every type is recorded: the comparison is of type and text)
        text = f"{type(e).__name__}: {e}".replace(fname, "<FILE>")
        return text if cut is None else text.replace(f"bytes={cut})", "bytes=<CUT>)")


def _calls(io, rec):
    calls = [("read", rec["read"]), ("end", io.index_record_end)]
    if rec["fourcc"] == b"IwSq":
        calls.append(("qtype", io.ivf_sq_qtype))
    return calls


def _cuts(length, bulk):
    """Every length 0 .. length - 1, less the interior of the bulk arrays [(start, stop)]: there the first, one middle and the last byte."""
    drop = set()
    for s, e in bulk:
        if e - s > 8:
            drop |= set(range(s + 2, e - 1)) - {(s + e) // 2}
    return [n for n in range(length) if n not in drop]


def _pokes(rec, variant, nlist, qn):
    """[(name, offset, bytes)]: the single-field overwrites of a record of this variant (offsets from the layout in index_io's docstring)."""
    C = 98 + 4 * qn * D                                          # the end of the centroids
    I = C + 9 + rec["middle"]                                    # 'ilar'
    u64, i32 = (lambda v: struct.pack("<Q", v)), (lambda v: struct.pack("<i", v))
    p = [("metric_type=1", 33, i32(1)), ("quantiser fourcc", 53, b"IxF2"), ("quantiser d", 57, i32(D + 1)), ("quantiser ntotal", 61, struct.pack("<q", nlist + 1)),
         ("quantiser metric=1", 86, i32(1)), ("nlist=0", 37, u64(0)), ("d=0", 4, i32(0)),
         ("direct-map type 1", C, b"\x01"), ("direct map of 3", C + 1, u64(3)),
         ("ilod", I, b"ilod"), ("ilar nlist + 1", I + 4, u64(nlist + 1)), ("ilar code_size + 1", I + 12, u64(struct.unpack_from("<Q", rec["bytes"][variant], I + 12)[0] + 1)),
         ("list sizes zzzz", I + 20, b"zzzz")]
    if variant == "sprs":                                        # the whole list goes to the plain record; the others get what only they can show
        return [("sprs odd words", I + 24, u64(3)), ("sprs cell = nlist", I + 32, u64(nlist)), ("sizes sum - 1", I + 40, u64(2))]
    if variant == "sprs2":
        return [("sprs cell twice", I + 48, u64(0))]
    if variant == "untrained":
        return [p[3]]
    p += [("full n_words + 1", I + 24, u64(nlist + 1)), ("sizes sum + 1", I + 32 + 8, u64(1))]
    if rec["fourcc"] == b"IwPQ":
        p += [("by_residual=2", C + 9, b"\x02"), ("code_size + 1", C + 10, u64(M + 1)), ("pq.d + 1", C + 18, u64(D + 1)), ("pq.M=3", C + 26, u64(3)),
              ("nbits=4", C + 34, u64(4)), ("codebook floats + 1", C + 42, u64(256 * D + 1))]
    if rec["fourcc"] == b"IwSq":
        T = C + 9 + 28                                           # the size word of `trained`
        n_t = struct.unpack_from("<Q", rec["bytes"][variant], T)[0]
        p += [("qtype=6", C + 9, i32(6)), ("qtype=1", C + 9, i32(1)), ("sq.d + 1", C + 21, u64(D + 1)), ("sq.code_size=99", C + 29, u64(99)),
              ("trained + 1", T, u64(n_t + 1)), ("code_size=99", T + 8 + 4 * n_t, u64(99)), ("by_residual=2", T + 16 + 4 * n_t, b"\x02")]
        for q in (0, 2, 4):                                      # the other two served quantisers in this record's place
            p.append((f"qtype={q}", C + 9, i32(q)))
    return p


def _bad_writes(io, f):
    """[(case, call)]: writer calls with wrong arguments, some wrong in two ways -- the first refusal stays the first."""
    cent, ids, sz = np.zeros((3, D), np.float32), np.arange(3), [2, 0, 1]
    rows, f16, u8 = np.zeros((3, D), np.float32), np.zeros((3, D), np.float16), np.zeros((3, D), np.uint8)
    pqc, t = np.zeros((M, 256, D // M), np.float32), np.zeros(2 * D, np.float32)
    return [("flat centroids", lambda: io.write_ivf_flat(f, cent[:2], sz, rows, ids)),
            ("flat ids", lambda: io.write_ivf_flat(f, cent, sz, rows, ids[:2])),
            ("flat centroids and ids", lambda: io.write_ivf_flat(f, cent[:2], sz, rows, ids[:2])),
            ("flat negative size", lambda: io.write_ivf_flat(f, cent, [4, -2, 1], rows, ids)),
            ("flat no cells", lambda: io.write_ivf_flat(f, cent[:0], [], rows[:0], ids[:0])),
            ("flat rows of d - 1", lambda: io.write_ivf_flat(f, cent, sz, rows[:, :3], ids)),
            ("flat ids and rows", lambda: io.write_ivf_flat(f, cent, sz, rows[:, :3], ids[:2])),
            ("pq centroids and codebooks", lambda: io.write_ivf_pq(f, cent[:2], pqc[:, :255], sz, u8[:, :M], ids)),
            ("pq codebooks", lambda: io.write_ivf_pq(f, cent, pqc[:, :255], sz, u8[:, :M], ids)),
            ("pq codebooks and codes", lambda: io.write_ivf_pq(f, cent, pqc[:, :255], sz, u8, ids)),
            ("pq codes", lambda: io.write_ivf_pq(f, cent, pqc, sz, u8, ids)),
            ("pq ids", lambda: io.write_ivf_pq(f, cent, pqc, sz, u8[:, :M], ids[:2])),
            ("pq codes and nprobe", lambda: io.write_ivf_pq(f, cent, pqc, sz, u8, ids, nprobe=-1)),
            ("sq centroids and codes", lambda: io.write_ivf_sq(f, cent[:2], sz, u8, ids)),
            ("sq codes of uint8", lambda: io.write_ivf_sq(f, cent, sz, u8, ids)),
            ("sq codes of 2 rows", lambda: io.write_ivf_sq(f, cent, sz, f16[:2], ids)),
            ("sq negative size", lambda: io.write_ivf_sq(f, cent, [4, -2, 1], f16, ids)),
            ("sq8 centroids and trained", lambda: io.write_ivf_sq8(f, cent[:2], t[:3], 0, sz, u8, ids)),
            ("sq8 trained", lambda: io.write_ivf_sq8(f, cent, t[:3], 0, sz, u8, ids)),
            ("sq8 trained of the other qtype", lambda: io.write_ivf_sq8(f, cent, t, 2, sz, u8, ids)),
            ("sq8 qtype 4", lambda: io.write_ivf_sq8(f, cent, t, 4, sz, u8, ids)),
            ("sq8 trained and codes", lambda: io.write_ivf_sq8(f, cent, t[:3], 0, sz, f16, ids)),
            ("sq8 codes of fp16", lambda: io.write_ivf_sq8(f, cent, t, 0, sz, f16, ids)),
            ("sq8 ids", lambda: io.write_ivf_sq8(f, cent, t, 0, sz, u8, ids[:2]))]


def derive(io, tmp):
    """-> (files {case: sha256}, reads {case: sha256 of the dump}, outcomes {(group, item): text}) with the index_io module `io`."""
    files, reads, outcomes = {}, {}, {}
    recs = records(io)
    f = os.path.join(tmp, "r.faiss")
    for case, call in _bad_writes(io, os.path.join(tmp, "w.faiss")):
        outcomes["writers", case] = outcome(call, f)
        assert not os.path.exists(os.path.join(tmp, "w.faiss")), case             # (a refused call replaces no file)

    def put(b):
        with open(f, "wb") as h:
            h.write(b)

    for name, rec in recs.items():
        rec["bytes"] = {}
        for variant, sizes in SIZES.items():
            rec["write"](f, sizes, variant != "untrained")
            with open(f, "rb") as h:
                b = rec["bytes"][variant] = h.read()
            files[f"{name} {variant}"] = hashlib.sha256(b).hexdigest()
            for call, fn in _calls(io, rec):
                reads[f"{name} {variant} {call}"] = outcome(lambda: fn(f), f)
            assert reads[f"{name} {variant} read"].startswith("ok "), (name, variant, reads[f"{name} {variant} read"])
            if rec["takes_offset"] and variant == "plain":
                rec["write"](f, sizes, variant != "untrained", prefix=PREFIX)
                with open(f, "rb") as h:
                    files[f"{name} {variant} prefix"] = hashlib.sha256(h.read()).hexdigest()
                for call, fn in _calls(io, rec):
                    reads[f"{name} {variant} prefix {call}"] = outcome(lambda: fn(f, len(PREFIX)), f)
                put(PREFIX + b + b"tail")                                            # a record inside a longer file: offset and end
                for call, fn in _calls(io, rec):
                    reads[f"{name} {variant} inside {call}"] = outcome(lambda: fn(f, len(PREFIX), len(PREFIX) + len(b)), f)
        if name.endswith("r0"):                                                  # (by_residual is one byte handed through: the damage goes to the r1 records)
            continue
        # every reader on every record (the fourcc and qtype refusals)
        put(rec["bytes"]["plain"])
        for other, orec in recs.items():
            if other.endswith("r1") or other == "flat":
                outcomes[f"{name} plain cross", other] = outcome(lambda: orec["read"](f), f)
        # truncations
        for variant in ("plain", "sprs"):
            b = rec["bytes"][variant]
            nlist = len(SIZES[variant])
            C = 98 + 4 * nlist * D + 9
            cuts = _cuts(len(b), [(98, 98 + 4 * nlist * D)] + [(C + s, C + e) for s, e in rec["bulk"]])
            for n in cuts:
                put(b[:n])
                for call, fn in _calls(io, rec):
                    outcomes[f"{name} {variant} cut {call}", n] = outcome(lambda: fn(f), f, n)
            if rec["takes_offset"]:
                put(PREFIX + b)
                for n in cuts:
                    for call, fn in _calls(io, rec):
                        outcomes[f"{name} {variant} cut-by-end {call}", n] = outcome(lambda: fn(f, len(PREFIX), len(PREFIX) + n), f, n)
        # single-field overwrites, and four trailing bytes
        for variant in ("plain", "sprs", "sprs2", "untrained"):
            b = rec["bytes"][variant]
            nlist = len(SIZES[variant])
            damaged = [(what, b[:at] + new + b[at + len(new):]) for what, at, new in _pokes(rec, variant, nlist, 0 if variant == "untrained" else nlist)]
            damaged.append(("four trailing bytes", b + b"\0\0\0\0"))
            for what, bad in damaged:
                assert len(bad) == len(b) + 4 * (what == "four trailing bytes")
                put(bad)
                for call, fn in _calls(io, rec):
                    outcomes[f"{name} {variant} poke {call}", what] = outcome(lambda: fn(f), f)
    return files, reads, outcomes


def pack(outcomes: dict) -> dict:
    """{(group, item): text} -> {text: {group: items}}; integer items as ranges "a-b,c", names joined by "|"."""
    by = {}
    for (group, item), text in outcomes.items():
        by.setdefault(text, {}).setdefault(group, []).append(item)
    out = {}
    for text, groups in sorted(by.items()):
        out[text] = {}
        for group, items in sorted(groups.items()):
            if isinstance(items[0], int):
                runs, items = [], sorted(items)
                for n in items:
                    if runs and runs[-1][1] == n - 1:
                        runs[-1][1] = n
                    else:
                        runs.append([n, n])
                out[text][group] = ",".join(str(a) if a == b else f"{a}-{b}" for a, b in runs)
            else:
                out[text][group] = "|".join(items)
    return out


def unpack(packed: dict) -> dict:
    out = {}
    for text, groups in packed.items():
        for group, items in groups.items():
            if " cut" in group:
                for run in items.split(","):
                    a, _, b = run.partition("-")
                    for n in range(int(a), int(b or a) + 1):
                        out[group, n] = text
            else:
                for item in items.split("|"):
                    out[group, item] = text
    return out


def main():
    import importlib.util                                       # index_io alone (it needs numpy only), not the package and its library
    spec = importlib.util.spec_from_file_location("index_io", os.path.join(os.path.dirname(os.path.dirname(HERE)), "lightretriever_amd", "index_io.py"))
    index_io = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(index_io)
    with tempfile.TemporaryDirectory() as tmp:
        files, reads, outcomes = derive(index_io, tmp)
    assert unpack(pack(outcomes)) == outcomes
    with open(OUT, "w") as h:
        json.dump(dict(files=files, reads=reads, outcomes=pack(outcomes)), h, indent=0, sort_keys=True)
        h.write("\n")
    print(f"{OUT}: {len(files)} files, {len(reads)} reads, {len(outcomes)} outcomes, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
