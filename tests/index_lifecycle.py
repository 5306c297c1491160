"""The index life-cycle check: what an index holds and returns is a function of its training and of the rows that are live,
in arrival order, and of nothing else that happened to it.

A helper module, no tests in it.  `Model` is the plain side: the training state of one family and `live`, the live rows in arrival order;
everything expected of the index at a checkpoint (`Model.expect`) is computed from those two alone, through the existing yardsticks -- no
score is implemented here.  `sequence(family, seed)` draws deterministic operation sequences that satisfy `conditions`; `NAMED` holds the
hand-written ones.  `Driver` is the GPU side: it applies the same operations to the family's index class and compares a checkpoint bit for
bit.  test_index_lifecycle_host.py checks the model, the generator and the op table without a GPU; test_gpu_index_lifecycle.py runs the
sequences.

Data (the recipes of ivf_store.Store, under which each yardstick gives the library's bits): integer rows in [-3, 3] for every family;
integer queries for the flat and fp16 stores, quarters for the 8-bit quantiser (whose decoded values lie on ivfsq8_yardstick.GRID_RANGES),
multiples of 2^-10 for the PQ and binary families (the table sums are the yardstick's own, the coarse scores exact); integer centroids."""
import os

import numpy as np

import binary_yardstick as YB
import ivf_range_yardstick as YR
import ivf_yardstick as IV
import ivfpq_yardstick as YPQ
import ivfsq8_yardstick as YS8
import ivfsq_yardstick as YSQ
import pq_yardstick as PQ
import graph_yardstick as G
import impact_yardstick as YI
import pca_yardstick as PCA
import range_codes_yardstick as RC
import refine_yardstick as RY
import sq8_yardstick as S8
from oracle import lrx_oracle as O

F32 = np.float32
D, NQ, NLIST, M_PQ = 64, 6, 8, 8
MAX_OPS, MAX_CHECKS, MAX_K, K_MID = 14, 6, 2048, 10
SEEDS = (0, 1, 2)
ID_BASE = 1000
EDGE_SIZES = (0, 1, 127, 128, 129)

# -- the op table ---------------------------------------------------------------------------------------------------------------------
# What an op needs of a class: it is served exactly where the class has every name (the host test asserts the table against hasattr).
OPS = ("add", "slot", "abandon", "reserve", "reset", "reload", "toggle", "refinalize", "check")
NEEDS = {"add": ("add",), "slot": ("append_slot", "commit"), "abandon": ("append_slot",), "reserve": ("reserve",), "reset": ("reset",),
         "reload": ("save", "load"), "toggle": ("_wants_shadow",), "refinalize": ("finalize",), "check": ("search",)}
_ALL = frozenset(OPS) - {"refinalize"}
_CODE = _ALL - {"toggle"}
_IVF = _ALL - {"toggle", "reserve"}


class Spec:
    def __init__(self, cls, kind, ops, blocked, big=(200, 900), max_live=2500, **kw):
        self.cls, self.kind, self.ops, self.blocked, self.big, self.max_live, self.kw = cls, kind, frozenset(ops), blocked, big, max_live, kw
        self.room = "slot" if kind in ("tiled", "refine", "graph") else "commit"


# kind: "tiled" / "code" / "ivf" (plain classes), "refine" / "pca" / "graph" (wrappers), "impact".  room (derived): what makes room for rows --
# append_slot, for the whole slot, or commit / add, for the committed rows.  blocked: the capacity is whole 128-row blocks.
SPECS = {
    "flat": Spec("FlatIPIndex", "tiled", _ALL, False),
    "sq_fp16": Spec("SQFp16Index", "tiled", _CODE, True),
    "pq": Spec("PQIndex", "code", _CODE, True),
    "sq8": Spec("SQ8Index", "code", _CODE, True, qtype="QT_8bit"),
    "sq8_uniform": Spec("SQ8Index", "code", _CODE, True, qtype="QT_8bit_uniform"),
    "binary": Spec("BinaryFlatIndex", "code", _CODE, True),
    "ivf_flat": Spec("IVFFlatIndex", "ivf", _IVF, False),
    "ivf_sq": Spec("IVFSQIndex", "ivf", _IVF, False, by_residual=True),
    "ivf_sq8": Spec("IVFSQ8Index", "ivf", _IVF, False, by_residual=True),
    "ivf_pq": Spec("IVFPQIndex", "ivf", _IVF, False, by_residual=True),
    "ivf_pq_raw": Spec("IVFPQIndex", "ivf", _IVF, False, by_residual=False),
    # RefineFlatIndex: a PQIndex base over a shadow-less FlatIPIndex store; an SQ8Index base over an SQFp16Index store
    "refine_pq_flat": Spec("RefineFlatIndex", "refine", _IVF, False),
    "refine_sq8_sq": Spec("RefineFlatIndex", "refine", _IVF, True),
    # PreTransformIndex: a fixed PCA state (128 -> 64) in front of a FlatIPIndex
    "pca_flat": Spec("PreTransformIndex", "pca", _IVF, False),
    # GraphFlatIndex: degree 8, every row an entry row; at most 600 rows (the yardstick's build is plain Python)
    "graph": Spec("GraphFlatIndex", "graph", _IVF, False, big=(100, 200), max_live=600),
    "impact": Spec("ImpactIndex", "impact", ("add", "reset", "refinalize", "check"), False),
}
FAMILIES = tuple(SPECS)
FLAT_CODE = ("flat", "sq_fp16", "pq", "sq8", "binary")
IVF = tuple(f for f in FAMILIES if SPECS[f].kind == "ivf")
WRAPPERS = ("refine_pq_flat", "refine_sq8_sq", "pca_flat", "graph")
HAS_RANGE = ("flat", "sq_fp16", "pq", "pca_flat", "impact") + IVF
HAS_RECONSTRUCT = tuple(f for f in FAMILIES if f not in ("flat", "impact"))
BASE_OF = {"sq8_uniform": "sq8", "ivf_flat": "flat", "ivf_sq": "sq_fp16", "ivf_sq8": "sq8", "ivf_pq": "pq", "ivf_pq_raw": "pq", "refine_pq_flat": "pq",
           "refine_sq8_sq": "sq8", "pca_flat": "flat", "graph": "flat"}
D_IN_PCA = 128
K_FACTOR = 2.0
GRAPH = dict(degree=8, intermediate_degree=16, ef_search=32, search_width=4, n_entry=600)


# -- sequences: ops are tuples ("add", n) ("slot", n, m) ("abandon", n) ("reserve", r) ("reset",) ("reload",) ("toggle", attr, value) ("check",),
#    and for the named ones ("add_cell", n, c) -- n rows that all fall in cell c -- and ("set_contents", n) -- n rows through set_contents ----
def _ceil128(n):
    return -(-n // 128) * 128


def simulate(family, ops):
    """One record per op: dict(op, before, after, realloc) -- ntotal before and after it, and whether it had to reallocate the row storage,
    by the classes' grow policy (index._grown: at least half as much again; load and set_contents leave capacity == ntotal)."""
    spec = SPECS[family]
    fit = _ceil128 if spec.blocked else (lambda n: n)
    n = cap = 0
    out = []
    for op in ops:
        before, realloc = n, False

        def room(need):
            nonlocal cap
            if need > cap:
                cap = fit(max(need, int(cap * 1.5) + 1))
                return True
            return False
        if op[0] in ("add", "add_cell"):
            realloc = op[1] > 0 and room(n + op[1])
            n += op[1]
        elif op[0] == "add_docs":
            n += len(op[1])
        elif op[0] == "slot":
            need = op[1] if spec.room == "slot" else op[2]
            realloc = need > 0 and room(n + need)
            n += op[2]
        elif op[0] == "abandon":
            realloc = spec.room == "slot" and room(n + op[1])
        elif op[0] == "reserve":
            if op[1] > cap:
                cap, realloc = fit(op[1]), True
        elif op[0] == "reset":
            n = 0
        elif op[0] == "reload":
            cap = fit(n)
        elif op[0] == "set_contents":
            n = op[1]
            cap = fit(n)
        out.append(dict(op=op, before=before, after=n, realloc=realloc, cap=cap))
    return out


def conditions(family, ops):
    """The issue's conditions on a generated sequence -> {name: bool}; every one must hold."""
    spec = SPECS[family]
    tr = simulate(family, ops)
    kinds = [o[0] for o in ops]
    checks = [i for i, k in enumerate(kinds) if k == "check"]
    c = {"length": len(ops) <= MAX_OPS and 1 <= len(checks) <= MAX_CHECKS, "live": max(t["after"] for t in tr) <= spec.max_live,
         "served": all(k in spec.ops for k in kinds), "ends_with_check": kinds[-1] == "check",
         "abandon_then_add": all(kinds[i + 1] == "add" for i, k in enumerate(kinds) if k == "abandon" and i + 1 < len(kinds)) and kinds[-1] != "abandon",
         "empty_check": any(tr[i]["after"] == 0 for i in checks),
         "three_full_checks": sum(tr[i]["after"] > 0 for i in checks) >= 3}
    # a reset followed by adds that end (at the next checkpoint) at fewer rows than before, inside a block that held rows before
    shrink = False
    for i, k in enumerate(kinds):
        nxt = next((j for j in checks if j > i), None)
        if k == "reset" and nxt is not None and "reset" not in kinds[i + 1:nxt]:
            shrink |= 0 < tr[nxt]["after"] < tr[i]["before"] and tr[nxt]["after"] % 128 != 0
    c["reset_shrinks"] = shrink
    if "reload" in spec.ops:              # (a class without persistence or slots -- the impact index -- has no storage of its own to regrow)
        c["realloc"] = any(t["realloc"] and t["before"] > 0 and t["before"] % 128 for t in tr)
        c["reload_then_add"] = any(k == "reload" and i + 1 < len(ops) and kinds[i + 1] == "add" and ops[i + 1][1] > 0 for i, k in enumerate(kinds))
    if "slot" in spec.ops:
        c["slot_partial"] = any(o[0] == "slot" and o[2] < o[1] for o in ops)
    if "refinalize" in spec.ops:          # an explicit finalize() with adds pending, and one with none
        c["refinalize_pending"] = any(k == "refinalize" and kinds[i - 1] == "add" for i, k in enumerate(kinds) if i)
        c["refinalize_idle"] = any(k == "refinalize" and kinds[i - 1] in ("check", "refinalize") for i, k in enumerate(kinds) if i)
    if spec.kind == "ivf":
        adds = lambda a, b: any(tr[j]["after"] > tr[j]["before"] for j in range(a, b))
        # a checkpoint directly after an add that follows an earlier checkpoint with rows: a sorted part and an unsorted tail
        c["sorted_and_tail"] = any(kinds[i - 1] == "add" and ops[i - 1][1] > 0 and any(j < i - 1 and tr[j]["after"] > 0 and "reset" not in kinds[j:i]
                                                                                      and "reload" not in kinds[j:i] for j in checks)
                                   for i in checks if i > 0)
        c["finalize_no_op"] = any(a + 1 == b or not adds(a + 1, b) for a, b in zip(checks, checks[1:]) if tr[a]["after"] > 0)
        c["empty_cell"] = any(0 < tr[i]["after"] < NLIST for i in checks)          # fewer rows than cells: one cell at least is empty
    return c


def features(family, ops):
    """What a sequence holds beyond the conditions -> {name: bool}: op values and op orders.  Seed s of a family must hold those that
    SEED_FEATURES[s % 3] names (as far as the class serves the ops), so that the three seeds between them issue an empty add, a slot that is
    committed whole, a reserve below, equal to and above ntotal on a non-empty index, and take reset, reload, slot and reserve in both orders."""
    tr = simulate(family, ops)
    kinds = [o[0] for o in ops]
    first = lambda k: kinds.index(k) if k in kinds else len(kinds)
    at = lambda k, ok: any(o[0] == k and ok(o, t) for o, t in zip(ops, tr))
    return {"add_0": at("add", lambda o, t: o[1] == 0 and t["before"] > 0),
            "slot_all": at("slot", lambda o, t: o[2] == o[1] > 0),
            "reserve_below": at("reserve", lambda o, t: o[1] < t["before"]),
            "reserve_equal": at("reserve", lambda o, t: o[1] == t["before"] > 0),
            "reserve_above": at("reserve", lambda o, t: t["realloc"] and t["before"] > 0),
            "reset_before_reload": first("reset") < first("reload") < len(kinds),
            "slot_after_reset": any(k == "slot" and i > first("reset") for i, k in enumerate(kinds)),
            "reserve_after_reload": any(k == "reserve" and i > first("reload") for i, k in enumerate(kinds)),
            "toggle": "toggle" in kinds, "toggle_shadow": any(o[:2] == ("toggle", "shadow_f16") for o in ops),
            "toggle_two_pass": any(o[:2] == ("toggle", "two_pass") for o in ops)}


SEED_FEATURES = {0: ("add_0", "reserve_below", "toggle_shadow"), 1: ("slot_all", "reserve_equal", "toggle_two_pass"),
                 2: ("reset_before_reload", "slot_after_reset", "reserve_after_reload", "reserve_above", "toggle")}
_FEATURE_OP = {"add_0": "add", "slot_all": "slot", "slot_after_reset": "slot", "reset_before_reload": "reload", "toggle": "toggle", "toggle_shadow": "toggle",
               "toggle_two_pass": "toggle"}


def wanted_features(family, seed):
    """The features seed `seed` of `family` must hold: those of SEED_FEATURES whose op the class serves."""
    return tuple(f for f in SEED_FEATURES[seed % 3] if _FEATURE_OP.get(f, "reserve") in SPECS[family].ops)


def _draw(family, rng, want):
    """One draw: the segments every sequence needs (rows and a checkpoint; a slot; a reload followed by an add; a reset followed by a few rows; for
    the inverted-file classes an add between two checkpoints and a checkpoint that follows another) in an order drawn from the rng, then filler
    ops -- reserves below / equal to / above ntotal, abandoned slots, toggles, empty and other adds, checkpoints, finalize() calls -- at
    positions drawn from the rng.  Nothing here makes the conditions hold: sequence() checks them and redraws."""
    spec = SPECS[family]
    has = lambda op: op in spec.ops
    ivf, impact = spec.kind == "ivf", spec.kind == "impact"
    big = lambda: int(rng.integers(spec.big[0], spec.big[1] + 1))
    edge = lambda: int(rng.choice(EDGE_SIZES[1:]))
    size = lambda: int(rng.choice([0, edge(), edge(), big()]))
    segs = [[("add", big()), C, ("add", edge()), C, C] if ivf else [("add", big()), C]]
    if not ivf:
        segs.append([("add", size()), C])
    if has("slot"):
        ns = big()
        segs.append([("slot", ns, int(rng.choice([0, ns // 2])))])
        if "slot_all" in want or rng.random() < 0.25:
            ns = int(rng.choice([edge(), big()]))
            segs.append([("slot", ns, ns)])
    if has("reload"):
        segs.append([("reload",), ("add", int(rng.choice([edge(), big()])))])
    if has("toggle"):
        segs.append([("toggle", str(rng.choice(["shadow_f16", "two_pass"])))])
    if impact:
        segs += [[("add", edge()), ("refinalize",)], [C, ("refinalize",)]]
    empty_after_reset = bool(rng.integers(2))           # the checkpoint on an empty index: straight after the reset, or before the first row
    small = int(rng.integers(1, NLIST)) if ivf else int(rng.integers(20, 128)) if impact else int(rng.integers(1, 256))
    segs.append([("reset",)] + ([C] if empty_after_reset else []) + [("add", small), C])
    ops = ([] if empty_after_reset else [C]) + [op for i in rng.permutation(len(segs)) for op in segs[i]]
    pool = [[("add", 0)], [("add", size())], [C]]
    if has("reserve"):
        pool += [[("reserve", "below")], [("reserve", "equal")], [("reserve", "above")]]
    if has("abandon"):
        pool.append([("abandon", big()), ("add", size())])
    if has("toggle"):
        pool += [[("toggle", "shadow_f16")], [("toggle", "two_pass")]]
    if has("refinalize"):
        pool.append([("refinalize",)])
    while len(ops) < MAX_OPS and rng.random() < 0.92:
        seg = pool[int(rng.integers(len(pool)))]
        pos = int(rng.integers(1, len(ops) + 1))
        if len(ops) + len(seg) > MAX_OPS or ops[pos - 1][0] == "abandon":     # (an abandoned slot stays directly in front of its add)
            continue
        ops[pos:pos] = seg
    if ops[-1] != C and len(ops) < MAX_OPS:
        ops.append(C)
    # reserves take their r from ntotal and the capacity where they stand, toggles flip what the (possibly reloaded) index has
    out, state = [], {}
    for op in ops:
        if op[0] == "reserve":
            tr = simulate(family, out)
            n, cap = (tr[-1]["after"], tr[-1]["cap"]) if tr else (0, 0)
            op = ("reserve", {"below": int(rng.integers(0, max(n, 1))), "equal": n, "above": 2 * cap + 129 + int(rng.integers(300))}[op[1]])
        elif op[0] == "toggle":
            state[op[1]] = not state.get(op[1], True)
            op = ("toggle", op[1], state[op[1]])
        elif op[0] == "reload":
            state = {}
        out.append(op)
    return out


def sequence(family, seed):
    """A deterministic pseudo-random op sequence of `family`: op kinds, their order and their sizes are drawn (_draw), checked against
    `conditions` and the seed's `wanted_features`, and redrawn until all of them hold."""
    rng = np.random.default_rng([FAMILIES.index(family), seed, 7])
    want = wanted_features(family, seed)
    for _ in range(20000):
        ops = _draw(family, rng, want)
        if all(conditions(family, ops).values()) and all(features(family, ops)[f] for f in want):
            return ops
    raise AssertionError(f"sequence({family!r}, {seed}): no draw satisfied the conditions")


# -- the named sequences: name -> (families, ops, ntotal at every checkpoint) --------------------------------------------------------------
C = ("check",)
NAMED = {
    # reset, then fewer rows than before, ending in the block that held rows 384 .. 399 before
    "reset_then_fewer_same_block": (FLAT_CODE + ("sq8_uniform",) + IVF, [("add", 400), C, ("reset",), ("add", 390), C], [400, 390]),
    # the same inside the first block, and down to one row
    "reset_then_one_row": (FLAT_CODE + IVF, [("add", 100), C, ("reset",), ("add", 1), C], [100, 1]),
    # a reserve that reallocates at ntotal = 129 (row 128 alone in its block), then up to 256
    "reserve_at_129_then_127": (FLAT_CODE, [("add", 129), ("reserve", 1000), ("add", 127), C], [256]),
    # reserves below and equal to ntotal on a non-empty index keep every block (300 rows: the third block is partial)
    "reserve_below_and_equal": (FLAT_CODE, [("add", 300), ("reserve", 172), ("reserve", 300), C, ("add", 1), C], [300, 301]),
    # empty adds, before and after a checkpoint
    "add_0_between_adds": (FLAT_CODE + IVF + WRAPPERS, [("add", 130), ("add", 0), C, ("add", 0), ("add", 1), C], [130, 131]),
    "slot_300_0_then_add_5": (FLAT_CODE + IVF, [("add", 60), ("slot", 300, 0), ("add", 5), C], [65]),
    "slot_300_150_then_slot_10_10": (FLAT_CODE + IVF, [("slot", 300, 150), C, ("slot", 10, 10), C], [150, 160]),
    "abandon_300_then_add_1": (FLAT_CODE + IVF, [("add", 130), ("abandon", 300), ("add", 1), C], [131]),
    "reload_empty_then_add": (FLAT_CODE + IVF, [("reload",), C, ("add", 129), C], [0, 129]),
    "reload_add_reload": (FLAT_CODE + IVF, [("add", 200), ("reload",), ("add", 100), ("reload",), C, ("add", 1), C], [300, 301]),
    # inverted-file: a sorted part and a one-row tail, then a search that rebuilds nothing
    "ivf_add_check_add1_check_check": (IVF, [("add", 300), C, ("add", 1), C, C], [300, 301, 301]),
    # rows through set_contents (capacity == ntotal afterwards), then an add that has to grow both the store and the cell numbers
    "ivf_set_contents_then_add": (IVF, [("set_contents", 200), C, ("add", 129), C], [200, 329]),
    # reset, then rows that all fall in cell 3: seven cells empty
    "ivf_reset_then_one_cell": (IVF, [("add", 300), C, ("reset",), ("add_cell", 40, 3), C], [300, 40]),
    # the rebuild replaces the PQ codes by a buffer of exactly two blocks; the next add grows from it
    "ivfpq_129_check_add1_check": (("ivf_pq", "ivf_pq_raw"), [("add", 129), C, ("add", 1), C], [129, 130]),
    # rows added without a shadow, a reserve that reallocates, the shadow switched on again: it is built for all of them
    "flat_shadow_off_reserve_on": (("flat",), [("add", 150), ("toggle", "shadow_f16", False), ("add", 200), ("reserve", 3000),
                                               ("toggle", "shadow_f16", True), ("add", 30), C], [380]),
    "flat_two_pass_off_then_on": (("flat",), [("add", 300), ("toggle", "two_pass", False), C, ("toggle", "two_pass", True), ("add", 20), C], [300, 320]),
    # reset with 400 shadowed rows behind it, 100 rows added without a shadow, the shadow switched on: it must be built, not taken as there
    "flat_reset_shadow_off_add_on": (("flat",), [("add", 400), C, ("reset",), ("toggle", "shadow_f16", False), ("add", 100), ("toggle", "shadow_f16", True), C],
                                     [400, 100]),
    # the wrappers over the same hand-written edges
    "wrapper_reset_then_fewer": (WRAPPERS, [("add", 300), C, ("reset",), ("add", 290), C], [300, 290]),
    "wrapper_slot_300_0_then_add_5": (WRAPPERS, [("add", 60), ("slot", 300, 0), ("add", 5), C], [65]),
    "wrapper_slot_300_150_then_slot_10_10": (WRAPPERS, [("slot", 300, 150), C, ("slot", 10, 10), C], [150, 160]),
    "wrapper_abandon_300_then_add_1": (WRAPPERS, [("add", 130), ("abandon", 300), ("add", 1), C], [131]),
    "wrapper_reload_empty_then_add": (WRAPPERS, [("reload",), C, ("add", 129), C], [0, 129]),
    "wrapper_reload_add_reload": (WRAPPERS, [("add", 200), ("reload",), ("add", 100), ("reload",), C, ("add", 1), C], [300, 301]),
    # the graph is rebuilt after a slot that commits rows, and not needed after one that commits none
    "graph_check_slot_check": (("graph",), [("add", 150), C, ("slot", 40, 20), C, ("slot", 40, 0), C], [150, 170, 170]),
    # reset, then as many rows as before: only the dropped table tells the index that its graph is stale
    "graph_reset_then_same_count": (("graph",), [("add", 150), C, ("reset",), ("add", 150), C], [150, 150]),
    # impact: documents 0 .. 2 over terms 0 .. 4, then a document with a new largest term id (9) and an empty one
    "impact_new_largest_term": (("impact",), [("add_docs", (((0, 2), (5, 1)), ((2, 4), (3, 7)), ((1,), (2,)))), C,
                                              ("add_docs", (((9, 0), (4, 6)), ((), ()))), C], [3, 5]),
    "impact_finalize_twice": (("impact",), [("add_docs", (((0, 3), (2, 9)), ((3,), (1,)))), ("refinalize",), ("refinalize",), C,
                                            ("add_docs", (((0,), (8,)),)), ("refinalize",), ("refinalize",), C], [2, 3]),
    # an add that brings no posting at all (one empty document) still makes finalize() run: the old postings stay
    "impact_empty_document_alone": (("impact",), [("add_docs", (((0, 3), (2, 9)), ((3,), (1,)))), C, ("add_docs", (((), ()),)), C], [2, 3]),
    "impact_reset_then_add": (("impact",), [("add", 200), C, ("reset",), C, ("add_docs", (((1, 0), (3, 4)), ((0,), (9,)))), C], [200, 0, 2]),
}


# -- the model ----------------------------------------------------------------------------------------------------------------------------
def _ids(I, mode, n):
    """The yardsticks' row numbers -> the ids the index reports in `mode`: "plain", "id_base" (ID_BASE + row) or "row_map" (row_map(n)[row])."""
    I = np.asarray(I, np.int64)
    if mode == "plain":
        return I
    return np.where(I < 0, -1, (ID_BASE + I) if mode == "id_base" else row_map(n)[np.maximum(I, 0)])


def row_map(n):
    return (3 * np.arange(max(n, 1), dtype=np.int64))[::-1].copy() + 11


def sq8_training_block(trained, uniform):
    """A fixed quarter-grid block whose column (or overall) minimum and maximum are vmin and vmin + vdiff of `trained`."""
    t = np.asarray(trained, F32)
    lo, hi = (np.full(D, t[0], F32), np.full(D, t[0] + t[1], F32)) if uniform else (t[:D], (t[:D] + t[D:]).astype(F32))
    mid = ((lo + hi) / 2).astype(F32)
    return np.stack([mid, lo, hi, mid])


class Model:
    """Training + live rows of one family.  reset() empties `live`, append() appends; nothing else changes it."""

    def __init__(self, family, seed=0, training=None):
        self.family, self.spec = family, SPECS[family]
        self.rng = rng = np.random.default_rng([FAMILIES.index(family), seed, 3])
        self.by_residual = self.spec.kw.get("by_residual")
        self.base = BASE_OF.get(family, family)          # what the codes are: the class's own, or the wrapper's base index's
        self.kind = self.spec.kind
        self.d_in = D_IN_PCA if self.kind == "pca" else D
        self.uniform = family == "sq8_uniform"
        if self.kind == "pca":                           # a fixed PCA state: 64 signed coordinates of the 128 (orthonormal rows), an integer offset
            cols = np.sort(rng.permutation(D_IN_PCA)[:D])
            self.A = np.zeros((D, D_IN_PCA), F32)
            self.A[np.arange(D), cols] = rng.choice([-1.0, 1.0], D)
            self.b = rng.integers(-2, 3, D).astype(F32)
        self.cent = rng.integers(-3, 4, (NLIST, D)).astype(F32) if self.spec.kind == "ivf" else None
        self.C = self.trained = None
        if self.base == "pq":
            self.C = rng.standard_normal((M_PQ, 256, D // M_PQ)).astype(F32)
            self.q = YB.grid_queries(rng, NQ, D)
        elif self.base == "sq8":
            r = np.array(YS8.GRID_RANGES, np.float64)[rng.integers(0, 3, 1 if self.uniform else D)]
            self.trained = np.concatenate([r[:, 0], r[:, 1]]).astype(F32)
            self.q = (rng.integers(-12, 13, (NQ, D)) / 4.0).astype(F32)
        elif self.base == "binary":
            self.q = YB.grid_queries(rng, NQ, D)
        else:
            self.q = rng.integers(-3, 4, (NQ, self.d_in)).astype(F32)
        if training is not None:
            vars(self).update(training)
        self.reset()

    # -- rows ----------------------------------------------------------------------------------------------------------------------
    def reset(self):
        self.live = np.zeros((0, self.d_in), F32)
        self.cells = np.zeros(0, np.int64)
        self._enc = None

    def draw(self, n):
        return self.rng.integers(-3, 4, (n, self.d_in)).astype(F32)

    def draw_in_cell(self, n, c):
        rows = np.zeros((0, D), F32)
        while len(rows) < n:
            x = self.draw(256)
            rows = np.concatenate([rows, x[IV.assign_cells(x, self.cent) == c]])
        return rows[:n]

    def filler(self, n):
        """Rows that are written into a slot and never committed: the largest norm the data can have, so that a bound, a shadow or a code
        that picked them up shows."""
        return np.full((n, self.d_in), 3, F32)

    def encode(self, x, cells=None):
        """The yardstick's encode of rows x (in their cells, for an inverted-file family): what the index -- a wrapper's base index -- stores
        of them; for the PCA wrapper, the reduced rows."""
        if len(x) == 0:
            return np.zeros((0, {"pq": M_PQ, "binary": D // 8}.get(self.base, D)), {"flat": F32, "sq_fp16": np.float16}.get(self.base, np.uint8))
        if self.kind == "pca":
            return PCA.apply(x, self.A, self.b).astype(F32)
        cent = self.cent if self.by_residual else None
        res = x if cent is None else YPQ.residuals(x, cent, cells)
        if self.base == "flat":
            return x.astype(F32)
        if self.base == "sq_fp16":
            return YSQ.encode(x, cent, cells if cent is not None else None)
        if self.base == "pq":
            return PQ.encode(res, self.C)
        if self.base == "sq8":
            return YS8.encode(x, self.trained, cent, cells if cent is not None else None)
        return YB.pack(x)

    def append(self, x):
        x = np.asarray(x, F32).reshape(-1, self.d_in)
        cells = IV.assign_cells(x, self.cent) if self.cent is not None else np.zeros(len(x), np.int64)
        enc = self.encode(x, cells)
        self._enc = enc if self._enc is None or len(self.live) == 0 else np.concatenate([self._enc, enc])
        self.live, self.cells = np.concatenate([self.live, x]), np.concatenate([self.cells, cells])

    @property
    def n(self):
        return len(self.live)

    def codes(self):
        """The encode of `live`, by ORIGINAL row (a row's code depends on the row and the training alone, so it is kept from append())."""
        return self.encode(self.live[:0]) if self._enc is None or self.n == 0 else self._enc

    def step(self, op):
        """Apply one op to the model -> the rows the index is handed by it (None where it is handed none)."""
        k = op[0]
        if k == "add":
            x = self.draw(op[1])
            self.append(x)
            return x
        if k == "add_cell":
            x = self.draw_in_cell(op[1], op[2])
            self.append(x)
            return x
        if k == "slot":
            x = np.concatenate([self.draw(op[2]), self.filler(op[1] - op[2])])
            self.append(x[:op[2]])
            return x
        if k == "abandon":
            return self.filler(op[1])
        if k == "set_contents":
            self.reset()
            x = self.draw(op[1])
            self.append(x)
            return x
        if k == "reset":
            self.reset()
        return None

    # -- what a checkpoint expects -----------------------------------------------------------------------------------------------------
    def decode(self, codes, cells):
        if len(codes) == 0:
            return np.zeros((0, D // 8), np.uint8) if self.base == "binary" else np.zeros((0, D), F32)
        cent = self.cent if self.by_residual else None
        if self.base == "flat":
            return codes
        if self.base == "sq_fp16":
            return YSQ.decode(codes, cent, cells if cent is not None else None)
        if self.base == "sq8":
            return YS8.decode(codes, self.trained, cent, cells if cent is not None else None)
        if self.base == "pq":
            y = YPQ.decode(codes, self.C).astype(F32)
            return y if cent is None else (cent[cells] + y).astype(F32)
        return codes                                                    # binary: reconstruct_n returns the packed bytes

    def ks(self):
        # (the re-ranking takes at most 2048 candidates: k_base = int(k * K_FACTOR))
        return sorted({1, K_MID, min(self.n + 3, int(MAX_K / K_FACTOR) if self.kind == "refine" else MAX_K)})

    def id_modes(self):
        # (the tiled classes apply row_map to the wire words of a sharded search only: their ids are plain or id_base)
        return ("plain", "id_base") if self.kind in ("tiled", "pca") else ("plain", "id_base", "row_map")

    def store_rows(self, x):
        """What a wrapper's row store gives back for rows x: the rows, or their fp16 codes decoded."""
        return YSQ.decode(YSQ.encode(x)) if self.family == "refine_sq8_sq" else x

    def graph(self):
        """The yardstick's table over the exact kNN lists of `live` (None when there are no rows)."""
        if self.n == 0:
            return None
        S = np.stack([IV.exact_scores(r, self.live) for r in self.live])
        return G.build_graph(G.knn_lists(S, GRAPH["intermediate_degree"]), GRAPH["degree"])

    def _search(self, k, nprobe, cell_order):
        q, codes = self.q, self.codes()
        if self.kind == "pca":
            return PCA.pre_transform_search(q, self.live, self.A, self.b, k)
        if self.kind == "refine":
            kb = RY.k_base(k, K_FACTOR)
            cand = (PQ.search(q, self.C, codes, kb) if self.base == "pq" else S8.search(q, codes, self.trained, kb))[1]
            return RY.rerank(q, self.store_rows(self.live), cand, k)
        if self.kind == "graph":
            Dw, Iw = np.full((NQ, k), -np.finfo(F32).max, F32), np.full((NQ, k), -1, np.int64)
            if self.n:
                beam, graph = max(GRAPH["ef_search"], k), self._graph
                for i in range(NQ):
                    row = IV.exact_scores(q[i], self.live)
                    entries = G.best_entries(row, G.entry_rows(self.n, min(self.n, GRAPH["n_entry"])), min(beam, self.n, 2048))
                    Iw[i], Dw[i] = G.beam_search(row, graph, entries, k, beam, GRAPH["search_width"])[:2]
            return Dw, Iw
        if self.spec.kind != "ivf":
            if self.base == "flat":
                return O.flat_ip_topk(q, self.live, k)
            if self.base == "sq_fp16":
                return PQ.topk(RC.sq_fp16_scores(q, codes), k)
            if self.base == "pq":
                return PQ.search(q, self.C, codes, k)
            if self.base == "sq8":
                return S8.search(q, codes, self.trained, k)
            return YB.search(q, codes, k, binary_k=self.binary_k(k))
        return self._ivf_fn()(*self._ivf_head(cell_order), *self._ivf_probes(nprobe), k)

    def binary_k(self, k):
        return max(k, 64)

    def _ivf_fn(self):
        return {"flat": IV.search, "sq_fp16": YSQ.search, "sq8": YS8.search, "pq": YPQ.search}[self.base]

    def _ivf_head(self, cell_order):
        row_ids, list_off = cell_order
        stored = self.codes()[row_ids]
        head = {"flat": (stored,), "sq_fp16": (stored,), "sq8": (stored, self.trained), "pq": (self.C, stored)}[self.base]
        return (self.q,) + head + (list_off, row_ids)

    def _ivf_probes(self, nprobe):
        probes = IV.probe_lists(self.q, self.cent, nprobe)
        if self.base == "flat":
            return (probes,)
        scores = np.stack([IV.exact_scores(self.q[i], self.cent[probes[i]]) for i in range(NQ)])
        return probes, scores, bool(self.by_residual)

    def expect(self):
        """Everything a checkpoint compares, from (training, live) alone."""
        n, codes = self.n, self.codes()
        e = dict(ntotal=n, live=self.live, codes=codes)
        order = None
        if self.spec.kind == "ivf":
            order = IV.cell_order(self.cells, NLIST)
            e.update(row_ids=order[0], list_off=order[1], list_sizes=np.diff(order[1]), stored=codes[order[0]])
        if self.kind in ("tiled", "refine", "pca", "graph"):                     # the rows of the tiled index itself, or of the wrapper's one
            tiled = codes if self.kind == "pca" else self.live
            e["tiled"] = tiled
            e["fp16"] = YSQ.encode(tiled)
            e["max_norm"] = float(np.sqrt((tiled.astype(np.float64) ** 2).sum(axis=1)).max()) if n else 0.0
        if self.kind == "graph":
            e["graph"] = self._graph = self.graph()
        i0 = max(0, (n - 1) // 128 * 128 - 5) if n else 0                        # a window across the last 128-row boundary, up to ntotal
        if self.kind == "pca":
            e["window"] = (i0, n - i0, PCA.reverse(codes[i0:], self.A, self.b).astype(F32))
        elif self.kind in ("refine", "graph"):
            e["window"] = (i0, n - i0, self.store_rows(self.live[i0:]))
        else:
            e["window"] = (i0, n - i0, self.decode(codes[i0:], self.cells[i0:]))
        e["search"] = []
        modes = self.id_modes()
        for nprobe in ((1, NLIST) if order else (None,)):
            for j, k in enumerate(self.ks()):
                Dw, Iw = self._search(k, nprobe, order)
                for mode in (modes if n and k == K_MID else (modes[j % len(modes)],)):
                    e["search"].append(dict(k=k, nprobe=nprobe, mode=mode, D=np.asarray(Dw, F32), I=_ids(Iw, mode, n)))
        if n == 0:
            for s in e["search"]:
                assert (s["I"] == -1).all() and (s["D"] == -np.finfo(F32).max).all()
        if self.family in HAS_RANGE and n:
            e["range"] = self._range(order)
        return e

    def _range(self, order):
        """(radius, mode, lims, D, I): the radius is the lowest score of the first query whose rows do not all score the same, so that
        query's result is neither empty nor everything (asserted whenever ntotal >= 2)."""
        n, q, codes = self.n, self.q, self.codes()
        if order is None:
            sq = PCA.apply(q, self.A, self.b).astype(F32) if self.kind == "pca" else q          # (the base is handed the reduced queries)
            S = {"flat": lambda: np.stack([IV.exact_scores(qi, codes) for qi in sq]),
                 "sq_fp16": lambda: RC.sq_fp16_scores(q, codes), "pq": lambda: RC.pq_scores(q, self.C, codes)}[self.base]()
            radius = self._radius(S)
            lims, Dw, Iw = RC.range_dense(S, radius, ID_BASE)
            scanned = np.full(NQ, n)
        else:
            probes = self._ivf_probes(NLIST)
            kw = {} if self.base == "flat" else dict(probe_scores=probes[1], by_residual=probes[2])
            head = self._ivf_head(order)[:-2]
            S = self._ivf_fn()(*self._ivf_head(order), *probes, n)[0]
            radius = self._radius(S)
            lims, Dw, Iw = YR.expected(self._ivf_fn(), head, probes[0], order[1], order[0], radius, id_base=ID_BASE, **kw)
            scanned = YR.scanned_rows(probes[0], order[1])
        assert n < 2 or YR.some_query_is_partial(lims, scanned), "the radius splits no query's rows"
        return dict(radius=radius, lims=lims, D=Dw, I=Iw)

    @staticmethod
    def _radius(S):
        for row in np.asarray(S, F32):
            if row.min() < row.max():
                return float(row.min())
        return float(np.asarray(S, F32).min())


class ImpactModel:
    """The impact index's model: `live` is the list of documents, (term ids, weights) each, in arrival order.  The postings, the term
    offsets and the largest weights are built here by hand from the documents; the scores are the yardstick's."""
    VOCAB = 40

    def __init__(self, family="impact", seed=0):
        self.family, self.spec, self.kind = family, SPECS[family], "impact"
        self.rng = rng = np.random.default_rng([FAMILIES.index(family), seed, 3])
        # query 0 asks for term 0, which most documents hold: whenever two of them do with different weights the range check splits it
        self.queries = [([0, 3], [1, 2])] + [(rng.choice(self.VOCAB, 4, replace=False).tolist(), rng.integers(1, 4, 4).tolist()) for _ in range(NQ - 1)]
        self.live, self.adds = [], 0

    n = property(lambda self: len(self.live))

    def draw(self, n):
        """n documents: term 0 (nine in ten) and up to five more of a vocabulary that grows with every add, weights 1 .. 50; one in ten is empty."""
        self.adds += 1
        docs = []
        for _ in range(n):
            if self.rng.integers(10) == 0:
                docs.append(([], []))
                continue
            t = [0] + (1 + self.rng.choice(self.VOCAB + 8 * self.adds - 1, int(self.rng.integers(0, 6)), replace=False)).tolist()
            docs.append((t, self.rng.integers(1, 51, len(t)).tolist()))
        return docs

    def step(self, op):
        if op[0] == "add":
            docs = self.draw(op[1])
        elif op[0] == "add_docs":
            docs = [(list(t), list(w)) for t, w in op[1]]
        else:
            if op[0] == "reset":
                self.live = []
            return None
        self.live = self.live + docs
        return docs

    def postings(self):
        """By hand: {term: [(row, weight), ...] in ascending row} over the live documents."""
        post = {}
        for row, (terms, weights) in enumerate(self.live):
            for t, w in zip(terms, weights):
                post.setdefault(int(t), []).append((row, int(w)))
        return post

    def expect(self):
        n, post = self.n, self.postings()
        n_terms = max(post) + 1 if post else 0
        sizes = np.array([len(post.get(t, ())) for t in range(n_terms)], np.int64)
        e = dict(ntotal=n, nnz=int(sizes.sum()), n_terms=n_terms, term_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                 maxw=np.array([max((w for _, w in post.get(t, ())), default=0) for t in range(n_terms)], np.int64),
                 postings=np.array([(r, w) for t in range(n_terms) for r, w in post.get(t, ())], np.int32).reshape(-1, 2), search=[])
        y = YI.Yardstick(*YI.csr_of(self.live))
        modes = ("plain", "id_base", "row_map")
        for j, k in enumerate(sorted({1, K_MID, min(n + 3, MAX_K)})):
            Dw, Iw = y.search(self.queries, k)
            for mode in (modes if n and k == K_MID else (modes[j % 3],)):
                e["search"].append(dict(k=k, nprobe=None, mode=mode, D=Dw, I=_ids(Iw, mode, n)))
        if n:
            S = RC.impact_scores(y, self.queries)
            radius = next((float(row[row >= 1].min()) for row in S if (row >= 1).any() and row[row >= 1].min() < row.max()), 0.0)
            lims, Dw, Iw = RC.range_impact(S, radius, ID_BASE)
            # (everything = all ntotal rows: a query whose hits all score the same still leaves out the rows it does not hit)
            assert n < 2 or YR.some_query_is_partial(lims, np.full(len(self.queries), n)), "the radius splits no query's rows"
            e["range"] = dict(radius=radius, lims=lims, D=Dw, I=Iw)
        return e


def make_model(family, seed=0):
    return ImpactModel(family, seed) if SPECS[family].kind == "impact" else Model(family, seed)


def replay(family, ops, seed=0):
    """The model alone over a sequence -> (model, the expectations of its checkpoints): the host side of a run."""
    m = make_model(family, seed)
    out = []
    for op in ops:
        m.step(op)
        if op[0] == "check":
            out.append(m.expect())
    return m, out


# -- the GPU side -------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    ne = _bits(got) != _bits(want)
    if ne.any():
        first = tuple(int(i) for i in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {first}: got {got[first]!r}, want {want[first]!r}")


class Driver:
    """One index of the model's family, taken through the same ops; check() compares it with Model.expect() bit for bit."""

    def __init__(self, model, tmp_path, trained=True):
        self.m, self.dir, self.nfile = model, str(tmp_path), 0
        self.idx = self.fresh(trained)

    def cls(self):
        import lightretriever_amd as A
        return getattr(A, self.m.spec.cls)

    def fresh(self, trained=True):
        """An empty index with the model's training, set without any k-means: set_contents on the empty index, or SQ8Index.train on the
        fixed quarter-grid block."""
        import torch
        m, cls, kw = self.m, self.cls(), self.m.spec.kw
        t = torch.from_numpy
        lo, ri = np.zeros(NLIST + 1, np.int64), np.zeros(0, np.int64)
        if m.family in ("flat", "sq_fp16", "binary"):
            return cls(D)
        if m.kind == "impact":
            return cls()
        if m.kind == "graph":
            return cls(D, **GRAPH)
        if m.kind == "pca":
            import lightretriever_amd as A
            st = dict(d_in=D_IN_PCA, d_out=D, eigen_power=0.0, random_rotation=False, is_trained=True, mean=np.zeros(D_IN_PCA, F32),
                      eigenvalues=np.ones(D_IN_PCA, F32), PCAMat=np.eye(D_IN_PCA, dtype=F32), A=m.A, b=m.b)
            return cls(A.PCAMatrix.from_state(st), A.FlatIPIndex(D))
        if m.kind == "refine":
            import lightretriever_amd as A
            if m.base == "pq":
                base = A.PQIndex(D, M_PQ)
                base.set_contents(t(m.C), torch.zeros(0, M_PQ, dtype=torch.uint8))
                return cls(base, k_factor=K_FACTOR)                      # (the default store: a FlatIPIndex without its shadow)
            base = A.SQ8Index(D, "QT_8bit")
            base.train(t(sq8_training_block(m.trained, False)))
            same(base.trained, m.trained, "SQ8Index.trained after train() on the grid block")
            return cls(base, A.SQFp16Index(D), k_factor=K_FACTOR)
        if m.family == "pq":
            idx = cls(D, M_PQ)
            if trained:
                idx.set_contents(t(m.C), torch.zeros(0, M_PQ, dtype=torch.uint8))
            return idx
        if m.base == "sq8" and m.spec.kind == "code":
            idx = cls(D, kw["qtype"])
            if trained:
                idx.train(t(sq8_training_block(m.trained, m.uniform)))
                same(idx.trained, m.trained, "SQ8Index.trained after train() on the grid block")
            return idx
        if m.family == "ivf_flat":
            idx = cls(D, NLIST)
            idx.set_contents(m.cent, torch.zeros(0, D), lo, ri)
        elif m.family == "ivf_sq":
            idx = cls(D, NLIST, by_residual=m.by_residual)
            idx.set_contents(m.cent, torch.zeros(0, D, dtype=torch.float16), lo, ri)
        elif m.family == "ivf_sq8":
            idx = cls(D, NLIST, "QT_8bit", by_residual=m.by_residual)
            idx.set_contents(m.cent, m.trained, torch.zeros(0, D, dtype=torch.uint8), lo, ri)
        else:
            idx = cls(D, NLIST, M_PQ, by_residual=m.by_residual)
            idx.set_contents(m.cent, m.C, torch.zeros(0, M_PQ, dtype=torch.uint8), lo, ri)
        return idx

    def apply(self, op):
        import torch
        rows = self.m.step(op)
        idx, k = self.idx, op[0]
        if k == "add_docs" or (k == "add" and self.m.kind == "impact"):
            idx.add(*YI.csr_of(rows))
        elif k in ("add", "add_cell"):
            idx.add(torch.from_numpy(rows))
        elif k in ("slot", "abandon"):
            idx.append_slot(op[1]).copy_(torch.from_numpy(rows))
            if k == "slot":
                idx.commit(op[2])
        elif k == "reserve":
            idx.reserve(op[1])
        elif k == "reset":
            idx.reset()
            if self.m.kind == "graph":
                assert idx.graph is None, "reset() left a graph"
        elif k == "refinalize":
            idx.finalize()
        elif k == "reload":
            self.nfile += 1
            f = os.path.join(self.dir, f"{self.m.family}_{self.nfile}.index")
            idx.save(f)
            self.idx = self.cls().load(f)
        elif k == "toggle":
            setattr(idx, op[1], op[2])
        elif k == "set_contents":
            row_ids, list_off = IV.cell_order(self.m.cells, NLIST)
            head = {"flat": (), "sq_fp16": (), "sq8": (self.m.trained,), "pq": (self.m.C,)}[self.m.base]
            idx.set_contents(self.m.cent, *head, torch.from_numpy(np.ascontiguousarray(self.m.codes()[row_ids])), list_off, row_ids)
        elif k == "check":
            self.check()
        if self.m.kind == "refine":                                  # base and store agree on ntotal after EVERY op
            assert self.idx.base_index.ntotal == self.idx.refine_index.ntotal == self.m.n, \
                f"after {op}: base {self.idx.base_index.ntotal} rows, store {self.idx.refine_index.ntotal}, model {self.m.n}"

    def run(self, ops):
        for op in ops:
            self.apply(op)

    # -- a checkpoint ----------------------------------------------------------------------------------------------------------------
    def _search(self, s):
        import torch
        idx, m = self.idx, self.m
        idx.id_base = ID_BASE if s["mode"] == "id_base" else 0
        kw = {}
        if s["mode"] == "row_map":
            kw["row_map"] = torch.from_numpy(row_map(m.n)).cuda()
        if s["nprobe"] is not None:
            kw["nprobe"] = s["nprobe"]
        try:
            if m.kind == "impact":
                from lightretriever_amd.impact_index import query_csr
                return idx.search(*query_csr(m.queries), s["k"], **kw)
            if m.base == "binary":
                kw["binary_k"] = m.binary_k(s["k"])
            return idx.search(torch.from_numpy(m.q), s["k"], **kw)
        finally:
            idx.id_base = 0

    def _range(self, radius):
        import torch
        idx, m = self.idx, self.m
        idx.id_base = ID_BASE
        try:
            if m.kind == "impact":
                from lightretriever_amd.impact_index import query_csr
                return idx.range_search(*query_csr(m.queries), radius)
            if m.kind == "ivf":
                return idx.range_search_probed(torch.from_numpy(m.q), radius, nprobe=NLIST)
            return idx.range_search(torch.from_numpy(m.q), radius)
        finally:
            idx.id_base = 0

    def _tiled(self, t, e, what):
        """A FlatIPIndex or SQFp16Index -- the class itself or a wrapper's store: rows, shadow / codes, and the bounds."""
        import torch
        if type(t).__name__ == "FlatIPIndex":
            same(t.vectors, e["tiled"], what + "vectors")
            if t.shadow_f16 and (len(e["tiled"]) or t._xb is not None):       # (an index that never held a row has allocated no shadow yet)
                same(t.shadow_rows(), e["fp16"], what + "shadow_rows()")
        else:
            same(t.codes(), e["fp16"], what + "codes()")
        b = t._bounds.cpu().numpy()
        assert float(b[0]) >= e["max_norm"], f"{what}_bounds[0] = {b[0]} below the largest live norm {e['max_norm']}"
        ref = type(t)(D)
        ref.shadow_f16 = getattr(t, "shadow_f16", True)
        ref.add(torch.from_numpy(e["tiled"]))
        same(t._bounds, ref._bounds.cpu().numpy(), what + "_bounds against a fresh index given the live rows in one add()")

    def check(self):
        idx, m = self.idx, self.m
        e = m.expect()
        fam, n = m.family, e["ntotal"]
        assert idx.ntotal == n, f"ntotal {idx.ntotal}, want {n}"
        for s in e["search"]:                                      # (first: a search is what makes a lazy structure current)
            Dg, Ig = self._search(s)
            what = f"search(k={s['k']}, nprobe={s['nprobe']}, ids={s['mode']})"
            same(Ig, s["I"], what + " ids")
            same(Dg, s["D"], what + " scores")
        if "range" in e:
            r = e["range"]
            for g, w, name in zip(self._range(r["radius"]), (r["lims"], r["D"], r["I"]), ("lims", "scores", "ids")):
                same(g, w, f"range search {name}")
        # contents
        if m.kind == "impact":
            assert (idx.nnz, idx.n_terms) == (e["nnz"], e["n_terms"]), f"nnz, n_terms = {idx.nnz}, {idx.n_terms}, want {e['nnz']}, {e['n_terms']}"
            same(idx.term_off_host, e["term_off"], "term_off_host")
            same(idx.maxw, e["maxw"], "maxw")
            same(idx._postings, e["postings"], "the postings, by (term, row)")
            return
        if m.kind == "tiled":
            self._tiled(idx, e, "")
        elif m.kind == "ivf":
            same(idx.row_ids, e["row_ids"], "row_ids")
            same(idx.list_off, e["list_off"], "list_off")
            same(idx.list_sizes, e["list_sizes"], "list_sizes")
            same(idx.stored_rows() if fam == "ivf_flat" else idx.stored_codes(), e["stored"], "the stored rows / codes")
        elif m.kind == "refine":
            same(idx.base_index.codes(), e["codes"], "the base's codes()")
            self._tiled(idx.refine_index, e, "the store's ")
        elif m.kind == "pca":
            self._tiled(idx.index, e, "the base's ")
        elif m.kind == "graph":
            self._tiled(idx.store, e, "the store's ")
            if n:
                same(idx.graph, e["graph"], "graph against build_graph over the exact kNN lists of the live rows")
            else:
                assert idx.graph is None or idx.graph.shape[0] == 0
        else:
            same(idx.codes(), e["codes"], "codes()")
        if fam in HAS_RECONSTRUCT:
            i0, cnt, want = e["window"]
            same(idx.reconstruct_n(i0, cnt), want, f"reconstruct_n({i0}, {cnt})")

