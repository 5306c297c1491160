"""Host-side mirror of the reference's searcher interfaces, dense branch only.

    FaissIndex          <- retriever/faiss_index.py:20-73      (build / search / reset over the HBM-resident FlatIPIndex)
    FlatIPFaissSearch   <- retriever/faiss_search.py:46-293, :477-510   (BEIR-style dense searcher)
    SQFaissSearch       <- retriever/faiss_search.py:567-611             (inner product; QT_fp16 over SQFp16Index, QT_8bit_uniform over SQ8Index)
    PQFaissSearch       <- retriever/faiss_search.py:326-383             (IndexPQ, 8-bit codes, inner product only, over PQIndex)
    FaissBinaryIndex    <- retriever/faiss_index.py:116-192              (Hamming candidates + float rerank over BinaryFlatIndex)
    BinaryFaissSearch   <- retriever/faiss_search.py:296-323             (IndexBinaryFlat, `dot` rerank only)
    PCAFaissSearch      <- retriever/faiss_search.py:512-565             (IndexPreTransform(PCAMatrix, base) over PreTransformIndex)
    RefineFaissSearch   (no counterpart in the reference)                (faiss IndexRefineFlat over a PQ / SQ / PCA base: RefineFlatIndex)
    IVFFaissSearch      (no counterpart in the reference)                (faiss IndexIVFFlat, inner product: IVFFlatIndex)
    IVFPQFaissSearch    (no counterpart in the reference)                (faiss IndexIVFPQ, inner product: IVFPQIndex)
    IVFSQFaissSearch    (no counterpart in the reference)                (faiss IndexIVFScalarQuantizer, QT_fp16, inner product: IVFSQIndex)
    IVFSQ8FaissSearch   (no counterpart in the reference)                (faiss IndexIVFScalarQuantizer, QT_8bit / QT_8bit_uniform, inner product: IVFSQ8Index)
    FaissHNSWIndex      <- retriever/faiss_index.py:76-113               (the wrapper's name; over GraphFlatIndex, no augmented dimension)
    HNSWFaissSearch     <- retriever/faiss_search.py:385-433             (a fixed-degree graph + beam search over GraphFlatIndex, not faiss's HNSW)
    HybridSearch        <- retriever/hybrid_search.py:25-403   (dense `den` / `emb` branches; `tok` / `spr` and their fusions with a sparse engine)
    ImpactSearch        <- retriever/anserini_search.py (AnseriniSearch's interface; impact search over ImpactIndex instead of Lucene)

Design differences, results preserved: corpus embeddings are encoded straight into the index shard (no CPU round trip, no
`index.add` copy); the per-chunk (score, pid) heaps of hybrid_search.py:182-205 are a running [Q, top_k] list kept on the
GPU and merged with lrx_merge_topk, so Python touches O(Q*k) values once at the end instead of once per corpus chunk.
`ignore_identical_ids` keeps the reference's order of operations (per-chunk top_k first, then the qid == pid hit is dropped).
Equal scores: inside one chunk (one index) the lower row wins (this build's IndexFlatIP contract); ACROSS
chunks the reference's heap compares (score, pid) tuples, so at equal scores the LARGER pid survives -- the running list is
therefore merged on keys that order the documents by descending pid.  Pinned by tests/golden/search_ref.json (outputs of the
reference's own HybridSearch.search / FlatIPFaissSearch.search).
"""
from __future__ import annotations

import logging
import os
import time
from typing import Optional

import numpy as np
import torch

from .impact_index import ImpactIndex, query_csr
from .graph import GraphFlatIndex
from .index import BinaryFlatIndex, FlatIPIndex, PQIndex, SQ8Index, SQFp16Index, merge_topk
from .sparse_rows import SparseRows, identity_term
from .ivf import IVFFlatIndex
from .ivfpq import IVFPQIndex
from .ivfsq import IVFSQIndex
from .ivfsq8 import IVFSQ8Index
from .refine import RefineFlatIndex, check_k_factor, check_k_base
from .transform import BASES as _PCA_BASES, PCAMatrix, PreTransformIndex

logger = logging.getLogger(__name__)
FLT_MAX = float(np.finfo(np.float32).max)


class FaissIndex:
    """`FaissIndex(index, passage_ids)` of the reference: search() maps row numbers through `_passage_ids` and logs QPS."""

    def __init__(self, index: FlatIPIndex, passage_ids: Optional[list] = None):
        self.index = index
        self._passage_ids = None if passage_ids is None else torch.as_tensor(np.asarray(passage_ids, dtype=np.int64), device=index.device)

    def _selector_index(self, what: str):
        """The wrapped index, if it takes a row selector (the four inverted-file indexes); TypeError otherwise."""
        if not isinstance(self.index, (IVFFlatIndex, IVFPQIndex, IVFSQIndex, IVFSQ8Index)):
            raise TypeError(f"FaissIndex.{what}(sel=...): {type(self.index).__name__} takes no row selector (the inverted-file indexes do)")
        return self.index

    def search(self, query_embeddings, k: int, sel=None, **kwargs):
        """sel: a RowSelector over the wrapped inverted-file index's rows (faiss SearchParameters(sel=...)): row numbers, not passage ids."""
        n = query_embeddings.shape[0]
        t0 = time.time()
        if sel is not None:
            scores, ids = self._selector_index("search").search(query_embeddings, k, sel=sel)
        else:
            scores, ids = self.index.search(query_embeddings, k)
        if self._passage_ids is not None:
            ids = torch.where(ids >= 0, self._passage_ids[ids.clamp(min=0)], ids)
        torch.cuda.synchronize(self.index.device)
        dt = max(time.time() - t0, 1e-9)
        logger.info("Num of queries: %d\tSearch time (s): %.3f\tQPS: %.3f", n, dt, n / dt)
        return scores, ids

    def range_search(self, query_embeddings, radius: float):
        """-> (lims, D, I) of FlatIPIndex.range_search, with I mapped through the passage ids as in search().  The wrapped index may be a
        FlatIPIndex, an SQFp16Index or a PQIndex: each serves range_search under its own score."""
        lims, scores, ids = self.index.range_search(query_embeddings, radius)
        if self._passage_ids is not None:
            ids = self._passage_ids[ids]
        return lims, scores, ids

    def range_search_probed(self, query_embeddings, radius: float, nprobe: Optional[int] = None, sel=None):
        """-> (lims, D, I) of the wrapped inverted-file index's range_search_probed (IVFFlatIndex, IVFPQIndex, IVFSQIndex, IVFSQ8Index): every
        row of each query's nprobe best cells with a score > radius, in segment order, I mapped through the passage ids as in range_search.
        sel: a RowSelector over the index's rows, as search() takes it."""
        if sel is not None:
            lims, scores, ids = self._selector_index("range_search_probed").range_search_probed(query_embeddings, radius, nprobe, sel=sel)
        else:
            lims, scores, ids = self.index.range_search_probed(query_embeddings, radius, nprobe)
        if self._passage_ids is not None:
            ids = self._passage_ids[ids]
        return lims, scores, ids

    @classmethod
    def build(cls, passage_ids: list, passage_embeddings, index: Optional[FlatIPIndex] = None, buffer_size: int = 50000):
        if index is None:
            index = FlatIPIndex(passage_embeddings.shape[1], capacity=len(passage_ids))
        for s in range(0, len(passage_ids), buffer_size):
            index.add(passage_embeddings[s:s + buffer_size])
        return cls(index, passage_ids)

    def save(self, fname: str):
        self.index.save(fname)     # faiss.write_index layout (index_io.py)

    def to_gpu(self):
        return self.index   # already HBM-resident; multi-GPU = one process per GPU (sharded.ShardedFlatIPIndex)

    def reset(self):
        self.index.reset()


class FaissBinaryIndex(FaissIndex):
    """`FaissBinaryIndex(index, passage_ids)` of the reference over a BinaryFlatIndex: search() binarises the queries with `threshold`, takes the
    Hamming top-`binary_k` and -- unless rerank=False, which returns the int32 Hamming lists -- rescores them with the float queries against
    the +-1 rows (BinaryFlatIndex.search); ids go through `_passage_ids`, QPS is logged.  The packed rows live in the index only (the
    reference keeps a second host copy for the rerank)."""

    def search(self, query_embeddings, k: int, binary_k: int = 1000, rerank: bool = True, score_function: str = "dot", threshold=0, **kwargs):
        n = query_embeddings.shape[0]
        t0 = time.time()
        scores, ids = self.index.search(query_embeddings, k, binary_k=binary_k, rerank=rerank, score_function=score_function, threshold=threshold)
        if self._passage_ids is not None:
            ids = torch.where(ids >= 0, self._passage_ids[ids.clamp(min=0)], ids)
        torch.cuda.synchronize(self.index.device)
        dt = max(time.time() - t0, 1e-9)
        logger.info("Num of queries: %d\tSearch time (s): %.3f\tQPS: %.3f", n, dt, n / dt)
        return scores, ids

    def range_search(self, query_embeddings, radius: float):
        raise NotImplementedError("FaissBinaryIndex.range_search is not served")

    @classmethod
    def build(cls, passage_ids: list, passage_embeddings, index: Optional[BinaryFlatIndex] = None, buffer_size: int = 50000):
        """passage_embeddings: floating [n, d] rows (binarised by the index) or uint8 [n, d / 8] packed rows, as the reference hands faiss."""
        if index is None:
            packed = str(passage_embeddings.dtype).endswith("uint8")
            index = BinaryFlatIndex(passage_embeddings.shape[1] * (8 if packed else 1), capacity=len(passage_ids))
        return super().build(passage_ids, passage_embeddings, index=index, buffer_size=buffer_size)


def _ids_and_list(queries):
    if isinstance(queries, dict):
        return list(queries.keys()), [queries[q] for q in queries]
    try:
        import datasets
        if isinstance(queries, datasets.Dataset):
            name = None
            for c in ["id", "_id", "query_id"]:
                if c in queries.column_names:
                    name = c
            if name is None:
                raise KeyError(f"No id column in queries dataset {queries.column_names}")
            return list(queries[name]), queries
    except ImportError:  # pragma: no cover
        pass
    raise NotImplementedError(f"Unrecognized type {type(queries)}")


def _sorted_corpus(corpus):
    """Longest text first (faiss_search.py:214-216 / hybrid_search.py:273-276); returns (corpus_ids, list of docs)."""
    if isinstance(corpus, dict):
        ids = sorted(corpus, key=lambda k: len(corpus[k].get("text", "")) if isinstance(corpus[k], dict) else len(corpus[k]), reverse=True)
        return ids, [corpus[c] for c in ids]
    try:
        import datasets
        if isinstance(corpus, datasets.Dataset):
            name = None
            for c in ["id", "_id", "docid", "doc_id"]:
                if c in corpus.column_names:
                    name = c
            if name is None:
                raise KeyError(f"No id column in corpus dataset {corpus.column_names}")
            rows = corpus.to_list()                      # one sequential read (row-by-row / permuted access costs ~30-90 us per document)
            rows.sort(key=lambda r: len(r["text"]), reverse=True)
            return [r[name] for r in rows], rows
    except ImportError:  # pragma: no cover
        pass
    raise NotImplementedError(f"Unrecognized type {type(corpus)}")


class DenseRetrievalFaissSearch:
    encode_kwargs: dict = {}           # extra arguments of the model's encode_corpus; HybridSearch(sparse_format="csr") sets them on its instance

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, use_single_gpu: bool = False,
                 use_multiple_gpu: bool = False, **kwargs):
        self.model = model       # provides encode_corpus() and encode_queries()
        self.batch_size = batch_size
        self.corpus_chunk_size = batch_size * 800 if corpus_chunk_size is None else corpus_chunk_size
        self.show_progress_bar = kwargs.get("show_progress_bar", True)
        self.convert_to_tensor = kwargs.get("convert_to_tensor", True)
        self.faiss_index: Optional[FaissIndex] = None
        self.use_single_gpu, self.use_multiple_gpu = use_single_gpu, use_multiple_gpu
        self.dim_size = None
        self.mapping, self.rev_mapping = {}, {}
        self.mteb_model_meta = None

    @classmethod
    def name(cls):
        return "faiss_search"

    def encode(self, sentences, batch_size, show_progress_bar=True, convert_to_tensor=True, **kwargs):
        return self.model.encode(sentences=sentences, batch_size=batch_size, show_progress_bar=show_progress_bar, convert_to_tensor=convert_to_tensor, **kwargs)

    def encode_queries(self, queries, batch_size, show_progress_bar=True, convert_to_tensor=True, **kwargs):
        return self.model.encode_queries(queries=queries, batch_size=batch_size, show_progress_bar=show_progress_bar, convert_to_tensor=convert_to_tensor, **kwargs)

    def encode_corpus(self, corpus, batch_size, show_progress_bar=True, convert_to_tensor=True, **kwargs):
        return self.model.encode_corpus(corpus=corpus, batch_size=batch_size, show_progress_bar=show_progress_bar, convert_to_tensor=convert_to_tensor, **kwargs)

    def _create_mapping_ids(self, corpus_ids):
        if not all(isinstance(d, int) for d in corpus_ids):
            for i, d in enumerate(corpus_ids):
                self.mapping[d] = i
                self.rev_mapping[i] = d

    def _clear(self):
        if self.faiss_index is not None:
            self.faiss_index.reset()
        self.faiss_index = None
        self.dim_size = None
        self.mapping, self.rev_mapping = {}, {}

    def index(self, corpus_emb, corpus_ids):
        raise NotImplementedError("Base class function. Please implement this depands on index type.")

    # -- persistence (faiss_search.py:99-123): {prefix}.{ext}.tsv id map + {prefix}.{ext}.faiss; one pair per rank ------------
    mapping_tsv_keys = ["beir-docid", "faiss-docid"]

    @staticmethod
    def _rank_world():
        import torch.distributed as dist
        return (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)

    def _load(self, input_dir: str, prefix: str, ext: str):
        from .index_io import load_tsv_to_dict, shard_prefix
        prefix = shard_prefix(prefix, *self._rank_world())
        self.mapping = load_tsv_to_dict(os.path.join(input_dir, "{}.{}.tsv".format(prefix, ext)), header=True)
        self.rev_mapping = {v: k for k, v in self.mapping.items()}
        return os.path.join(input_dir, "{}.{}.faiss".format(prefix, ext)), sorted(self.rev_mapping)

    def save(self, output_dir: str, prefix: str, ext: str):
        from .index_io import save_dict_to_tsv, shard_prefix
        prefix = shard_prefix(prefix, *self._rank_world())
        os.makedirs(output_dir, exist_ok=True)
        save_dict_to_tsv(self.mapping, os.path.join(output_dir, "{}.{}.tsv".format(prefix, ext)), keys=self.mapping_tsv_keys)
        path = os.path.join(output_dir, "{}.{}.faiss".format(prefix, ext))
        self.faiss_index.save(path)
        logger.info("Index size: {:.2f}MB".format(os.path.getsize(path) * 0.000001))

    # -- device-level retrieval used by the chunk loop ---------------------------------------------------------------
    def _retrieve_device(self, query_emb, top_k: int):
        return self.faiss_index.search(_as_device(query_emb, self.faiss_index.index.device), top_k)

    def retrieve_with_emb(self, query_emb, query_ids: list, top_k: int, **kwargs) -> dict:
        """-> {qid: {pid: score}} (faiss_search.py:143-173).  Rows beyond the index size (id -1) are dropped."""
        scores, ids = self._retrieve_device(query_emb, top_k)
        return _to_result_dict(scores, ids, query_ids, self.rev_mapping)

    def search(self, corpus, queries, top_k: int = 1000, score_function: str = None, return_sorted: bool = False,
               ignore_identical_ids: bool = False, **kwargs) -> dict:
        query_ids, queries_list = _ids_and_list(queries)
        q = self.model.encode_queries(queries_list, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                                      convert_to_tensor=self.convert_to_tensor)
        if isinstance(q, dict):
            q = q["dense_reps"] if "dense_reps" in q else q["emb_reps"]
        return _chunked_dense_search(self, q, query_ids, corpus, top_k, ignore_identical_ids)


class FlatIPFaissSearch(DenseRetrievalFaissSearch):
    index_cls = FlatIPIndex          # the shard type every index / load builds
    index_ext = "flat"               # the default `ext` of load / save: files {prefix}.{ext}.faiss / .tsv
    serves_rpc_shards = True         # _chunked_dense_search may place the shards on the reference's RPC workers (rpc_shards: FlatIPIndex)
    faiss_index_cls = FaissIndex     # the (index, passage_ids) wrapper that search() goes through

    def _new_index(self, dim: int, capacity: int):
        return self.index_cls(dim, capacity=capacity)

    def _train(self, idx, corpus_emb):
        """index(): fit a fresh shard that needs training to the chunk before its rows are added (nothing to fit for a flat shard)."""

    def index(self, corpus_emb, corpus_ids):
        """Index already-encoded embeddings (Tensor on any device / ndarray) -- faiss_search.py:490-504."""
        self._create_mapping_ids(corpus_ids)
        self.dim_size = corpus_emb.shape[1]
        rows = [self.mapping.get(c, c) for c in corpus_ids]
        idx = self._new_index(corpus_emb.shape[1], len(rows))
        self._train(idx, corpus_emb)
        self.faiss_index = self.faiss_index_cls.build(rows, corpus_emb, index=idx)

    def _index_in_place(self, docs: list, corpus_ids: list, dim: int):
        """Encode a corpus chunk straight into a fresh shard (embeddings never leave HBM)."""
        self._create_mapping_ids(corpus_ids)
        self.dim_size = dim
        idx = self._new_index(dim, len(docs))
        if not docs:                                  # a rank without a batch in this chunk: empty shard, searches return padding
            self.faiss_index = self.faiss_index_cls(idx, None)
            return None
        slot = idx.append_slot(len(docs))
        enc = emb = self.model.encode_corpus(docs, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                                             convert_to_tensor=True, out=slot, **self.encode_kwargs)
        if isinstance(emb, dict):
            emb = emb["dense_reps"]
        if emb.data_ptr() != slot.data_ptr():       # a model that does not support `out=`: one device copy
            slot.copy_(emb.to(slot.device))
        idx.commit(len(docs))
        self.faiss_index = self.faiss_index_cls(idx, [self.mapping.get(c, c) for c in corpus_ids])
        return enc if isinstance(enc, dict) else {"dense_reps": enc}   # what encode_corpus returned (sparse_reps ride along)

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        """faiss_search.py:478-488: id map + index file -> HBM shard of this rank."""
        path, passage_ids = self._load(input_dir, prefix, self.index_ext if ext is None else ext)
        idx = self.index_cls.load(path)
        if passage_ids and len(passage_ids) != idx.ntotal:
            raise ValueError(f"{path}: {idx.ntotal} rows but {len(passage_ids)} ids in the map")
        self.dim_size = idx.d
        self.faiss_index = self.faiss_index_cls(idx, passage_ids or None)

    def save(self, output_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        super().save(output_dir, prefix, self.index_ext if ext is None else ext)

    def get_index_name(self):
        return "flat_faiss_index"


def _inner_product_only(who: str, similarity_metric) -> None:
    """The refusal of every searcher that takes a similarity_metric: only inner product is served."""
    if similarity_metric not in (0, "METRIC_INNER_PRODUCT", "ip"):     # faiss.METRIC_INNER_PRODUCT == 0
        raise NotImplementedError(f"{who}: similarity_metric {similarity_metric!r} is not served (only inner product, faiss.METRIC_INNER_PRODUCT = 0)")


class SQFaissSearch(FlatIPFaissSearch):
    """faiss_search.py:567-611: IndexScalarQuantizer(d, quantizer_type, METRIC_INNER_PRODUCT).  "QT_fp16" (the default) is served by
    SQFp16Index -- 2 B/element resident, exact inner products of the fp32 query with the decoded codes -- and "QT_8bit_uniform" by SQ8Index:
    1 B/element, one trained range for all dimensions, index() trains on the chunk and then adds it (FaissTrainIndex.build), _index_in_place
    trains when the staging slot is committed.  index / _index_in_place / save behave like FlatIPFaissSearch's with that shard; load() picks
    the shard class from the file's qtype, as faiss.read_index would, whatever the constructor said.
    "QT_8bit" (a range per dimension) is REFUSED by this constructor although SQ8Index serves it: an existing test pins the refusal.  It is
    reachable through SQ8Index(d, "QT_8bit"), torch.ops.lrx.sq8_ip_topk, the C API and load() of a QT_8bit file; lifting the refusal (together
    with that test) is a one-line follow-up.  Other quantizer types and metrics are not served; neither are shards on RPC workers."""
    index_cls = SQFp16Index
    index_ext = "sq"
    serves_rpc_shards = False

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, similarity_metric=0, quantizer_type: str = "QT_fp16",
                 **kwargs):
        if quantizer_type not in ("QT_fp16", "QT_8bit_uniform"):
            raise NotImplementedError(f"SQFaissSearch: quantizer_type {quantizer_type!r} is not served (only 'QT_fp16' and 'QT_8bit_uniform')")
        _inner_product_only("SQFaissSearch", similarity_metric)
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.similarity_metric = 0
        self.qname = quantizer_type
        if quantizer_type != "QT_fp16":
            self.index_cls = SQ8Index

    def _new_index(self, dim: int, capacity: int):
        if self.index_cls is SQ8Index:
            return SQ8Index(dim, self.qname, capacity=capacity)
        return super()._new_index(dim, capacity)

    def _train(self, idx, corpus_emb):
        if isinstance(idx, SQ8Index):
            idx.train(corpus_emb)                     # index() trains on the chunk, then adds it (FaissTrainIndex.build)

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        """The shard class follows the file's qtype (4: SQFp16Index, 0 / 2: SQ8Index), as faiss.read_index would."""
        from .index_io import QT_FP16, shard_prefix, sq_qtype
        e = self.index_ext if ext is None else ext
        path = os.path.join(input_dir, "{}.{}.faiss".format(shard_prefix(prefix, *self._rank_world()), e))
        self.index_cls = SQFp16Index if sq_qtype(path) == QT_FP16 else SQ8Index
        super().load(input_dir, prefix, ext)
        self.qname = "QT_fp16" if self.index_cls is SQFp16Index else self.faiss_index.index.qtype

    def get_index_name(self):
        return "sq_faiss_index"


class PQFaissSearch(FlatIPFaissSearch):
    """faiss_search.py:326-383: IndexPQ(d, num_of_centroids, code_size, METRIC_INNER_PRODUCT), served by PQIndex -- num_of_centroids is
    faiss's M (sub-quantisers, M bytes per row), code_size its nbits.  index() trains on the chunk and then adds it (FaissTrainIndex.build);
    _index_in_place trains on the encoded chunk when its staging slot is committed.  Not served: OPQ (use_rotation), the L2 metric,
    code_size != 8, shards on RPC workers."""
    index_cls = PQIndex
    index_ext = "pq"
    serves_rpc_shards = False

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, num_of_centroids: int = 96, code_size: int = 8,
                 similarity_metric=0, use_rotation: bool = False, **kwargs):
        if use_rotation:
            raise NotImplementedError("PQFaissSearch: use_rotation (OPQ) is not served")
        _inner_product_only("PQFaissSearch", similarity_metric)
        if code_size != 8:
            raise NotImplementedError(f"PQFaissSearch: code_size (nbits) {code_size} is not served (only 8)")
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.num_of_centroids = num_of_centroids
        self.code_size = code_size
        self.use_rotation = False
        self.similarity_metric = 0

    def _new_index(self, dim: int, capacity: int) -> PQIndex:
        if dim % self.num_of_centroids:
            raise ValueError(f"PQFaissSearch: dimension {dim} is not a multiple of num_of_centroids={self.num_of_centroids}")
        return PQIndex(dim, self.num_of_centroids, self.code_size, capacity=capacity)

    def _train(self, idx: PQIndex, corpus_emb):
        idx.train(corpus_emb)                         # index() trains on the chunk, then adds it (faiss_search.py:370-383 via FaissTrainIndex.build)

    def get_index_name(self):
        return "pq_faiss_index"


class BinaryFaissSearch(FlatIPFaissSearch):
    """faiss_search.py:296-323: IndexBinaryFlat(d) over the binarised embeddings (bit j = x[j] > threshold[j]), searched through FaissBinaryIndex --
    the Hamming top-`binary_k` rescored with the float queries against the +-1 rows.  d / 8 bytes per row resident.  index / _index_in_place /
    load / save behave like FlatIPFaissSearch's with a BinaryFlatIndex shard.  Every retrieval of the chunk loop is the rerank search, so per-chunk
    scores are fp32 and merge like any other searcher's.  Not served: score_function "cos_sim" (a per-query rescale of the same ranking), shards
    on RPC workers."""
    index_cls = BinaryFlatIndex
    index_ext = "bin"
    serves_rpc_shards = False
    faiss_index_cls = FaissBinaryIndex

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, binary_k: int = 1000, threshold=0,
                 score_function: str = "dot", **kwargs):
        if score_function != "dot":
            raise NotImplementedError(f"BinaryFaissSearch: score_function {score_function!r} is not served (only 'dot')")
        if not 1 <= int(binary_k) <= BinaryFlatIndex.MAX_K:
            raise ValueError(f"BinaryFaissSearch: binary_k={binary_k} out of range (1..{BinaryFlatIndex.MAX_K})")
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.binary_k = int(binary_k)
        self.threshold = threshold
        self.score_function = score_function

    def _new_index(self, dim: int, capacity: int) -> BinaryFlatIndex:
        return BinaryFlatIndex(dim, capacity=capacity, threshold=self.threshold)

    def _retrieve_device(self, query_emb, top_k: int):
        if top_k > self.binary_k:
            raise ValueError(f"BinaryFaissSearch: top_k={top_k} > binary_k={self.binary_k} (the rerank sees binary_k candidates; raise binary_k, at most "
                             f"{BinaryFlatIndex.MAX_K})")
        return self.faiss_index.search(_as_device(query_emb, self.faiss_index.index.device), top_k, binary_k=self.binary_k, rerank=True,
                                       score_function=self.score_function, threshold=self.threshold)

    def search(self, corpus, queries, top_k: int = 1000, score_function: str = None, **kwargs) -> dict:
        if top_k > self.binary_k:
            raise ValueError(f"BinaryFaissSearch: top_k={top_k} > binary_k={self.binary_k}")
        if score_function not in (None, "dot"):
            raise NotImplementedError(f"BinaryFaissSearch: score_function {score_function!r} is not served (only 'dot')")
        return super().search(corpus, queries, top_k=top_k, score_function=score_function, **kwargs)

    def get_index_name(self):
        return "binary_faiss_index"


class PCAFaissSearch(FlatIPFaissSearch):
    """faiss_search.py:512-565: IndexPreTransform(PCAMatrix(d, output_dimension, eigen_power, random_rotation), base_index), served by
    PreTransformIndex -- the dense rows are reduced to output_dimension by an exact fp32 linear map on their way into the base index, the
    queries on their way into its search.  base_index: a FlatIPIndex, SQFp16Index, SQ8Index or PQIndex of dimension output_dimension, used
    (and emptied first) for every chunk, or None: a fresh FlatIPIndex(output_dimension) per chunk.  As in the reference the matrix trained
    on the first chunk is kept in `pca_matrix` and copied (PCAMatrix.copy_from) into the index of every later chunk, so the chunk loop
    trains once and the scores of different chunks are comparable; pass pca_matrix= to start from a trained one.  index() trains on the chunk
    and then adds it, _index_in_place trains when the staging slot is committed.  Not served: random_rotation, shards on RPC workers."""
    index_cls = PreTransformIndex
    index_ext = "pca"
    serves_rpc_shards = False

    def __init__(self, model, base_index=None, output_dimension: Optional[int] = None, batch_size: int = 128, corpus_chunk_size: Optional[int] = None,
                 pca_matrix: Optional[PCAMatrix] = None, random_rotation: bool = False, eigen_power: float = 0.0, **kwargs):
        if output_dimension is None or int(output_dimension) < 1:
            raise ValueError(f"PCAFaissSearch: output_dimension={output_dimension!r} must be a positive integer (the dimension after the PCA)")
        if random_rotation:
            raise NotImplementedError("PCAFaissSearch: random_rotation is not served (faiss's random rotation cannot be reproduced)")
        if base_index is not None and not isinstance(base_index, _PCA_BASES):
            raise TypeError(f"PCAFaissSearch: base index {type(base_index).__name__} is not served (only "
                            f"{', '.join(c.__name__ for c in _PCA_BASES)})")
        if base_index is not None and base_index.d != int(output_dimension):
            raise ValueError(f"PCAFaissSearch: the base index's d={base_index.d} is not output_dimension={output_dimension}")
        if pca_matrix is not None and not isinstance(pca_matrix, PCAMatrix):
            raise TypeError(f"PCAFaissSearch: pca_matrix must be a PCAMatrix, got {type(pca_matrix).__name__}")
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.base_index = base_index
        self.output_dim = int(output_dimension)
        self.pca_matrix = pca_matrix
        self.random_rotation = False
        self.eigen_power = float(eigen_power)

    def _new_index(self, dim: int, capacity: int) -> PreTransformIndex:
        pca = PCAMatrix(dim, self.output_dim, self.eigen_power, self.random_rotation)
        if self.pca_matrix is not None:
            pca.copy_from(self.pca_matrix)
        self.pca_matrix = pca                         # (trained with the index it belongs to: index() / the commit of _index_in_place)
        base = self.base_index
        if base is None:
            base = FlatIPIndex(self.output_dim, capacity=capacity)
        else:
            base.reset()
        return PreTransformIndex(pca, base)

    def _train(self, idx: PreTransformIndex, corpus_emb):
        idx.train(corpus_emb)                         # index() trains on the chunk, then adds it (FaissTrainIndex.build)

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        super().load(input_dir, prefix, ext)
        self.pca_matrix = self.faiss_index.index.transform
        self.output_dim, self.eigen_power = self.pca_matrix.d_out, self.pca_matrix.eigen_power

    def get_index_name(self):
        return "pca_faiss_index"


class _IVFFaissSearch(FlatIPFaissSearch):
    """What the four inverted-file searchers share: nlist / nprobe and their refusal, the clamp of both to a chunk, training on the chunk
    before its rows are added, and a load() that takes the parameters back from the file.  A subclass refuses the metric and its own
    arguments first, then hands nlist / nprobe to this constructor."""
    serves_rpc_shards = False
    loaded: dict = {}                # load(): attribute of the searcher <- attribute of the loaded index, besides nlist and nprobe

    def __init__(self, model, batch_size, corpus_chunk_size, nlist: int, nprobe: int, **kwargs):
        if nlist < 1 or nprobe < 1:
            raise ValueError(f"{type(self).__name__}: nlist={nlist} and nprobe={nprobe} must be >= 1")
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.nlist, self.nprobe = int(nlist), int(nprobe)
        self.similarity_metric = 0

    def _cells(self, capacity: int):
        """-> (nlist, nprobe) of a shard of `capacity` rows."""
        nlist = max(1, min(self.nlist, capacity))     # a chunk of fewer rows than nlist: one cell per row at the most
        return nlist, min(self.nprobe, nlist, 2048)

    def _train(self, idx, corpus_emb):
        idx.train(corpus_emb)                         # index() trains on the chunk, then adds it

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        super().load(input_dir, prefix, ext)
        idx = self.faiss_index.index
        self.nlist, self.nprobe = idx.nlist, idx.nprobe
        for mine, theirs in self.loaded.items():
            setattr(self, mine, getattr(idx, theirs))


class IVFPQFaissSearch(_IVFFaissSearch):
    """faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, num_of_centroids, code_size, METRIC_INNER_PRODUCT) as a searcher, served by IVFPQIndex: every
    chunk is clustered into nlist k-means cells (at most its row count), its rows are stored as num_of_centroids bytes of PQ codes (of their
    residuals to the cell's centroid with by_residual) and a search scans the codes of each query's nprobe best cells.  num_of_centroids is
    faiss's M and code_size its nbits, as in PQFaissSearch, whose refusals apply (code_size != 8, any metric but inner product).  index() trains
    on the chunk and then adds it; _index_in_place trains on the encoded chunk when its staging slot is committed.  load() takes nlist, nprobe,
    M and by_residual from the file.  Not served: the L2 metric, shards on RPC workers."""
    index_cls = IVFPQIndex
    index_ext = "ivfpq"
    loaded = dict(num_of_centroids="M", by_residual="by_residual")

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, nlist: int = 1024, nprobe: int = 32,
                 num_of_centroids: int = 96, code_size: int = 8, by_residual: bool = True, similarity_metric=0, **kwargs):
        _inner_product_only("IVFPQFaissSearch", similarity_metric)
        if code_size != 8:
            raise NotImplementedError(f"IVFPQFaissSearch: code_size (nbits) {code_size} is not served (only 8)")
        super().__init__(model, batch_size, corpus_chunk_size, nlist, nprobe, **kwargs)
        if num_of_centroids < 1:                      # (after nlist / nprobe, which the base refuses before it sets anything up)
            raise ValueError(f"IVFPQFaissSearch: num_of_centroids={num_of_centroids} must be >= 1")
        self.num_of_centroids, self.code_size, self.by_residual = int(num_of_centroids), code_size, bool(by_residual)

    def _new_index(self, dim: int, capacity: int) -> IVFPQIndex:
        if dim % self.num_of_centroids:
            raise ValueError(f"IVFPQFaissSearch: dimension {dim} is not a multiple of num_of_centroids={self.num_of_centroids}")
        nlist, nprobe = self._cells(capacity)
        return IVFPQIndex(dim, nlist, self.num_of_centroids, self.code_size, nprobe=nprobe, by_residual=self.by_residual,
                          capacity=capacity)

    def get_index_name(self):
        return "ivfpq_faiss_index"


class IVFSQFaissSearch(_IVFFaissSearch):
    """faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, quantizer_type, METRIC_INNER_PRODUCT) as a searcher, served by IVFSQIndex: every
    chunk is clustered into nlist k-means cells (at most its row count), its rows are stored as fp16 codes (of their residuals to the cell's
    centroid with by_residual) and a search scans the codes of each query's nprobe best cells, every scanned row scored exactly over its code.
    quantizer_type: only "QT_fp16" (the 8-bit types are IVFSQ8FaissSearch's).  index() trains on the chunk and then adds it; _index_in_place trains on the encoded chunk when its staging
    slot is committed.  load() takes nlist, nprobe and by_residual from the file.  Not served: other quantiser types, the L2 metric, shards on
    RPC workers."""
    index_cls = IVFSQIndex
    index_ext = "ivfsq"
    loaded = dict(by_residual="by_residual")

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, nlist: int = 1024, nprobe: int = 32,
                 quantizer_type: str = "QT_fp16", by_residual: bool = True, similarity_metric=0, **kwargs):
        _inner_product_only("IVFSQFaissSearch", similarity_metric)
        if quantizer_type != "QT_fp16":
            raise NotImplementedError(f"IVFSQFaissSearch: quantizer_type {quantizer_type!r} is not served (only 'QT_fp16')")
        super().__init__(model, batch_size, corpus_chunk_size, nlist, nprobe, **kwargs)
        self.quantizer_type, self.by_residual = quantizer_type, bool(by_residual)

    def _new_index(self, dim: int, capacity: int) -> IVFSQIndex:
        nlist, nprobe = self._cells(capacity)
        return IVFSQIndex(dim, nlist, self.quantizer_type, nprobe=nprobe, by_residual=self.by_residual, capacity=capacity)

    def get_index_name(self):
        return "ivfsq_faiss_index"


class IVFSQ8FaissSearch(_IVFFaissSearch):
    """faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit | QT_8bit_uniform, METRIC_INNER_PRODUCT) ("IVF...,SQ8") as a searcher, served by
    IVFSQ8Index: every chunk is clustered into nlist k-means cells (at most its row count), the range of the 8-bit quantiser is trained on the
    chunk's residuals (its rows without by_residual), the rows are stored as 1-byte codes and a search scans the codes of each query's nprobe best
    cells, every scanned row scored exactly over its decoded code.  quantizer_type: "QT_8bit" or "QT_8bit_uniform" ("QT_fp16" is
    IVFSQFaissSearch's).  index() trains on the chunk and then adds it; _index_in_place trains on the encoded chunk when its staging slot is
    committed.  load() takes nlist, nprobe, quantizer_type and by_residual from the file.  Not served: other quantiser types, the L2 metric,
    shards on RPC workers."""
    index_cls = IVFSQ8Index
    index_ext = "ivfsq8"
    loaded = dict(quantizer_type="qtype", by_residual="by_residual")

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, nlist: int = 1024, nprobe: int = 32,
                 quantizer_type: str = "QT_8bit", by_residual: bool = True, similarity_metric=0, **kwargs):
        _inner_product_only("IVFSQ8FaissSearch", similarity_metric)
        if quantizer_type == "QT_fp16":
            raise NotImplementedError("IVFSQ8FaissSearch: quantizer_type 'QT_fp16' is served by IVFSQFaissSearch (faiss_search_map='ivfsq')")
        if quantizer_type not in ("QT_8bit", "QT_8bit_uniform"):
            raise NotImplementedError(f"IVFSQ8FaissSearch: quantizer_type {quantizer_type!r} is not served (only 'QT_8bit' and 'QT_8bit_uniform')")
        super().__init__(model, batch_size, corpus_chunk_size, nlist, nprobe, **kwargs)
        self.quantizer_type, self.by_residual = quantizer_type, bool(by_residual)

    def _new_index(self, dim: int, capacity: int) -> IVFSQ8Index:
        nlist, nprobe = self._cells(capacity)
        return IVFSQ8Index(dim, nlist, self.quantizer_type, nprobe=nprobe, by_residual=self.by_residual, capacity=capacity)

    def get_index_name(self):
        return "ivfsq8_faiss_index"


class RefineFaissSearch(FlatIPFaissSearch):
    """faiss IndexRefineFlat(base) / IndexRefine(base, IndexScalarQuantizer(QT_fp16)) as a searcher, served by RefineFlatIndex: every chunk is
    indexed twice -- into a lossy base shard and into a full-precision row store -- and searched in two stages: the base's top
    int(top_k * k_factor) rows, rescored exactly from the store, best top_k.  refine_base: "pq", "sq", "pca", "ivfpq", "ivfsq" or "ivfsq8" -- the searcher (PQFaissSearch,
    SQFaissSearch, PCAFaissSearch, IVFPQFaissSearch, IVFSQFaissSearch, IVFSQ8FaissSearch) whose shard is the base; its own arguments go through **kwargs unchanged, so its refusals (use_rotation,
    QT_8bit, random_rotation, ...) apply unchanged, and so does PCAFaissSearch's reuse of the first chunk's matrix.  refine_type: "flat" (fp32
    rows without a shadow, 4 B/element) or "fp16" (SQFp16Index codes, 2 B/element).  index / _index_in_place / load / save behave like
    FlatIPFaissSearch's with that shard; load() takes k_factor and the shard classes from the file.  Not served: shards on RPC workers."""
    index_cls = RefineFlatIndex
    index_ext = "refine"
    serves_rpc_shards = False
    BASE_SEARCHERS = {"pq": PQFaissSearch, "sq": SQFaissSearch, "pca": PCAFaissSearch, "ivfpq": IVFPQFaissSearch, "ivfsq": IVFSQFaissSearch,
                      "ivfsq8": IVFSQ8FaissSearch}

    def __init__(self, model, refine_base: Optional[str] = None, k_factor: float = 1.0, refine_type: str = "flat", batch_size: int = 128,
                 corpus_chunk_size: Optional[int] = None, **kwargs):
        if refine_base not in self.BASE_SEARCHERS:
            raise ValueError(f"RefineFaissSearch: refine_base={refine_base!r} must be one of {sorted(self.BASE_SEARCHERS)}")
        if refine_type not in ("flat", "fp16"):
            raise ValueError(f"RefineFaissSearch: refine_type={refine_type!r} must be 'flat' or 'fp16'")
        self.k_factor = check_k_factor(k_factor)
        # held only to build and train base shards (_new_index / _train); it never indexes or searches itself
        self.base_search = self.BASE_SEARCHERS[refine_base](model, batch_size=batch_size, corpus_chunk_size=corpus_chunk_size, **kwargs)
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.refine_base, self.refine_type = refine_base, refine_type

    def _new_index(self, dim: int, capacity: int) -> RefineFlatIndex:
        base = self.base_search._new_index(dim, capacity)
        if self.refine_type == "fp16":
            store = SQFp16Index(dim, capacity=capacity)
        else:
            store = FlatIPIndex(dim, capacity=capacity)
            store.shadow_f16 = False                  # gathered, never streamed: 4 B/element instead of 6
        return RefineFlatIndex(base, store, k_factor=self.k_factor)

    def _train(self, idx: RefineFlatIndex, corpus_emb):
        self.base_search._train(idx.base_index, corpus_emb)

    def _retrieve_device(self, query_emb, top_k: int):
        check_k_base(top_k, self.k_factor, "RefineFaissSearch")
        return super()._retrieve_device(query_emb, top_k)

    def search(self, corpus, queries, top_k: int = 1000, score_function: str = None, **kwargs) -> dict:
        check_k_base(top_k, self.k_factor, "RefineFaissSearch")
        return super().search(corpus, queries, top_k=top_k, score_function=score_function, **kwargs)

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        super().load(input_dir, prefix, ext)
        idx = self.faiss_index.index
        self.k_factor = idx.k_factor
        self.refine_type = "fp16" if isinstance(idx.refine_index, SQFp16Index) else "flat"
        if isinstance(idx.base_index, PreTransformIndex) and isinstance(self.base_search, PCAFaissSearch):
            self.base_search.pca_matrix = idx.base_index.transform

    def get_index_name(self):
        return "refine_faiss_index"


class IVFFaissSearch(_IVFFaissSearch):
    """faiss IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) as a searcher, served by IVFFlatIndex: every chunk is clustered into
    nlist k-means cells (at most its row count) and a search scans the rows of each query's nprobe best cells, scored exactly.  index() trains
    on the chunk and then adds it; _index_in_place trains on the encoded chunk when its staging slot is committed.  index / load / save behave
    like FlatIPFaissSearch's with that shard; load() takes nlist and nprobe from the file.  Not served: the L2 metric, shards on RPC workers."""
    index_cls = IVFFlatIndex
    index_ext = "ivf"

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, nlist: int = 1024, nprobe: int = 32, similarity_metric=0,
                 **kwargs):
        _inner_product_only("IVFFaissSearch", similarity_metric)
        super().__init__(model, batch_size, corpus_chunk_size, nlist, nprobe, **kwargs)

    def _new_index(self, dim: int, capacity: int) -> IVFFlatIndex:
        nlist, nprobe = self._cells(capacity)
        return IVFFlatIndex(dim, nlist, nprobe=nprobe, capacity=capacity)

    def get_index_name(self):
        return "ivf_faiss_index"



class FaissHNSWIndex(FaissIndex):
    """`FaissHNSWIndex(index, passage_ids)` of the reference over a GraphFlatIndex.  The reference appends a dimension to every row (and a zero to
    every query) so that faiss's L2 HNSW ranks by inner product; none is needed here: the graph is built and searched under the inner product
    itself.  The two agree on the neighbourhoods exactly when all rows have one norm -- what the encoder emits (normalised embeddings)."""

    @classmethod
    def build(cls, passage_ids: list, passage_embeddings, index: Optional[GraphFlatIndex] = None, buffer_size: int = 50000):
        return super().build(passage_ids, passage_embeddings, GraphFlatIndex(passage_embeddings.shape[1]) if index is None else index, buffer_size)


class HNSWFaissSearch(FlatIPFaissSearch):
    """faiss_search.py:385-433 (IndexHNSWFlat(d + 1, hnsw_store_n) with efSearch / efConstruction) as a searcher, served by GraphFlatIndex: a
    fixed-degree neighbour graph built from exact kNN lists and searched by a beam search (the shape faiss itself runs on a GPU, GpuIndexCagra),
    not faiss's sequential HNSW insertion.  The arguments keep the reference's names and defaults and map as follows:
      degree              = min(2 * hnsw_store_n, 64) rounded down to a multiple of 8, at least 8 (faiss's level-0 degree is 2 M; the reference's
                            default of 1024 neighbours is clamped, logged once)
      intermediate_degree = min(max(hnsw_ef_construction, 2 * degree), 256)
      ef_search           = hnsw_ef_search
    and both degrees are clamped to a chunk's row count.  index / _index_in_place / save behave like FlatIPFaissSearch's with that shard (the
    graph is built at the chunk's first search); load() takes the parameters back from the file.  No augmented dimension (FaissHNSWIndex).
    Not served: the L2 metric, shards on RPC workers, faiss's HNSW file record."""
    index_cls = GraphFlatIndex
    index_ext = "hnsw"
    serves_rpc_shards = False
    faiss_index_cls = FaissHNSWIndex
    _clamp_logged = False

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, hnsw_store_n: int = 512, hnsw_ef_search: int = 128,
                 hnsw_ef_construction: int = 200, similarity_metric=0, **kwargs):
        _inner_product_only("HNSWFaissSearch", similarity_metric)
        if hnsw_store_n < 1 or hnsw_ef_construction < 1 or not 1 <= hnsw_ef_search <= 2048:
            raise ValueError(f"HNSWFaissSearch: hnsw_store_n={hnsw_store_n} and hnsw_ef_construction={hnsw_ef_construction} must be >= 1, "
                             f"hnsw_ef_search={hnsw_ef_search} in 1 .. 2048")
        super().__init__(model, batch_size, corpus_chunk_size, **kwargs)
        self.hnsw_store_n, self.hnsw_ef_search, self.hnsw_ef_construction = int(hnsw_store_n), int(hnsw_ef_search), int(hnsw_ef_construction)
        self.similarity_metric = 0
        if 2 * self.hnsw_store_n > 64 and not HNSWFaissSearch._clamp_logged:
            HNSWFaissSearch._clamp_logged = True
            logger.info("HNSWFaissSearch: hnsw_store_n=%d (level-0 degree %d) is served with graph degree 64", self.hnsw_store_n, 2 * self.hnsw_store_n)

    def _degrees(self, capacity: Optional[int] = None):
        """-> (degree, intermediate_degree) of a shard of `capacity` rows (None: unclamped)."""
        degree = max(8, min(2 * self.hnsw_store_n, 64) // 8 * 8)
        K = min(max(self.hnsw_ef_construction, 2 * degree), 256)
        if capacity is not None:                      # a chunk of fewer rows than a degree: lists as long as the chunk, the table at least 8 wide
            degree = max(8, min(degree, capacity) // 8 * 8)
            K = max(degree, min(K, capacity))
        return degree, K

    def _new_index(self, dim: int, capacity: int) -> GraphFlatIndex:
        degree, K = self._degrees(capacity)
        return GraphFlatIndex(dim, degree=degree, intermediate_degree=K, ef_search=self.hnsw_ef_search, capacity=capacity)

    def load(self, input_dir: str, prefix: str = "my-index", ext: Optional[str] = None):
        super().load(input_dir, prefix, ext)
        idx = self.faiss_index.index
        self.hnsw_store_n, self.hnsw_ef_search, self.hnsw_ef_construction = idx.degree // 2, idx.ef_search, idx.intermediate_degree

    def get_index_name(self):
        return "hnsw_faiss_index"


class ImpactSearch:
    """The sparse engine HybridSearch calls, with the reference's AnseriniSearch interface (`index(corpus_emb, corpus_ids)`,
    `retrieve_with_emb(query_emb, query_ids, top_k)`, `_clear()`), over an HBM-resident ImpactIndex instead of Lucene behind a JVM: impact
    search (`-impact -pretokenized`) of a JsonVectorCollection -- the contract of include/lrx.h (lrx_impact_search), DESIGN §5.4.6.
    Documents are {term: integer weight} dicts, queries {term: count} dicts or pseudo text ("tok tok tok ...": split on whitespace and
    counted).  Terms are strings -- token ids as strings, tokens, the empty-vector marker "-1" (an ordinary term) -- numbered in first-seen
    order by `vocab`; query terms no document has brought are dropped.  A document is a row in insertion order (an id indexed twice is two
    rows); equal scores rank the earlier row first.  BM25 (`anserini_impact_search=False`) and other collections are not served.

    Documents and queries may also be a SparseRows (device CSR of token ids, sparse_rows.py): the three arrays go to the ImpactIndex as they
    are, no Python object per posting.  The first index() call of a kind fixes the numbering of the engine -- dicts: `vocab`; SparseRows: the
    identity rule, token id i is term i and the empty-vector marker is term vocab_size (`identity_term` maps host queries the same way) --
    until _clear() followed by a call of the other kind.  Mixing the kinds on a non-empty engine raises ValueError.  Every query form is
    served under either numbering and gives the same hits."""

    def __init__(self, model=None, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, **kwargs):
        if not kwargs.get("anserini_impact_search", True):
            raise NotImplementedError("ImpactSearch: anserini_impact_search=False (BM25) is not served, only impact search")
        vector_type = kwargs.get("anserini_vector_type", "JsonVectorCollection")
        if vector_type != "JsonVectorCollection":
            raise NotImplementedError(f"ImpactSearch: anserini_vector_type={vector_type!r} is not served (only 'JsonVectorCollection')")
        self.model = model
        self.batch_size = batch_size
        self.corpus_chunk_size = corpus_chunk_size
        self.vocab: dict = {}              # term -> int32 id, first-seen order; survives _clear() like a tokenizer would
        self.impact_index = ImpactIndex()
        self.rev_mapping: list = []        # row -> pid
        self.identity_vocab_size: Optional[int] = None   # None: terms are numbered by `vocab`; V: the identity rule over V token ids

    @classmethod
    def name(cls):
        return "impact_search"

    def _clear(self):
        self.impact_index.reset()
        self.rev_mapping = []

    def index(self, corpus_emb, corpus_ids):
        """corpus_emb: a list of {term: weight} dicts (the JsonVectorCollection `vector` field); appended to the index, the GPU is not touched
        before the first retrieval."""
        assert len(corpus_emb) == len(corpus_ids)
        if isinstance(corpus_emb, SparseRows):
            return self._index_rows(corpus_emb, corpus_ids)
        if self.rev_mapping and self.identity_vocab_size is not None:
            raise ValueError("ImpactSearch.index: dicts after SparseRows on a non-empty engine (one numbering per engine: _clear() first)")
        self.identity_vocab_size = None
        vocab = self.vocab
        off = np.zeros(len(corpus_emb) + 1, dtype=np.int64)
        terms, weights = [], []
        for i, doc in enumerate(corpus_emb):
            for t, w in doc.items():
                if int(w) != w:
                    raise ValueError(f"ImpactSearch.index: weight {w!r} of term {t!r} is not an integer (impact search scores quantised weights)")
                terms.append(vocab.setdefault(t, len(vocab)))
                weights.append(int(w))
            off[i + 1] = len(terms)
        self.impact_index.add(np.asarray(terms, dtype=np.int64), np.asarray(weights, dtype=np.int64), off)
        self.rev_mapping += list(corpus_ids)

    def _index_rows(self, rows: SparseRows, corpus_ids):
        """A SparseRows of documents: the identity numbering, the arrays handed to the index where they are."""
        if self.rev_mapping and self.identity_vocab_size is None:
            raise ValueError("ImpactSearch.index: SparseRows after dicts on a non-empty engine (one numbering per engine: _clear() first)")
        if self.rev_mapping and self.identity_vocab_size != rows.vocab_size:
            raise ValueError(f"ImpactSearch.index: SparseRows over {rows.vocab_size} token ids, the engine holds rows over {self.identity_vocab_size}")
        self.impact_index.add(rows.terms, rows.weights, rows.row_off)
        self.identity_vocab_size = rows.vocab_size
        self.rev_mapping += list(corpus_ids)

    def _term_id(self, term: str) -> Optional[int]:
        if self.identity_vocab_size is not None:
            return identity_term(term, self.identity_vocab_size)
        return self.vocab.get(term)

    def _query_rows(self, rows: SparseRows) -> tuple:
        """A SparseRows of queries (weights are counts) -> (q_off, q_term, q_cnt) for ImpactIndex.search.  Under the identity numbering of the
        same vocabulary the arrays are the answer; else the token ids are renumbered on the host like the string terms they stand for."""
        if self.identity_vocab_size == rows.vocab_size:
            return rows.row_off, rows.terms, rows.weights
        off, term, cnt = rows.row_off.cpu().numpy(), rows.terms.cpu().numpy().astype(np.int64), rows.weights.cpu().numpy()
        lut = np.full(rows.vocab_size + 1, -1, dtype=np.int64)
        if self.identity_vocab_size is not None:     # identity over another vocabulary size: shared token ids keep their number
            n = min(rows.vocab_size, self.identity_vocab_size)
            lut[:n] = np.arange(n)
            lut[rows.vocab_size] = self.identity_vocab_size
        else:
            for t, i in self.vocab.items():
                j = identity_term(t, rows.vocab_size)
                if j is not None:
                    lut[j] = i
        mapped = lut[term]
        keep = mapped >= 0
        new_off = np.zeros(off.size, dtype=np.int64)
        np.add.at(new_off, np.repeat(np.arange(off.size - 1), np.diff(off))[keep] + 1, 1)
        return np.cumsum(new_off), mapped[keep], cnt[keep]

    def _query_terms(self, query):
        """One query -> (term ids, counts): pseudo text is split and counted, unknown terms are dropped."""
        if isinstance(query, str):
            from collections import Counter
            query = Counter(query.split())
        pairs = [(i, c) for i, c in ((self._term_id(t), c) for t, c in query.items()) if i is not None]
        for _, c in pairs:
            if int(c) != c:
                raise ValueError(f"ImpactSearch: query count {c!r} is not an integer")
        return [t for t, _ in pairs], [int(c) for _, c in pairs]

    def retrieve_with_emb(self, query_emb, query_ids, top_k: int, **kwargs):
        """query_emb: per query a {term: count} dict or pseudo text, or one SparseRows of queries (weights are counts) -> {qid: {pid: score}}
        of the top_k hits (documents sharing a term)."""
        assert len(query_emb) == len(query_ids)
        csr = self._query_rows(query_emb) if isinstance(query_emb, SparseRows) else query_csr([self._query_terms(q) for q in query_emb])
        D, I = self.impact_index.search(*csr, top_k)
        return _to_result_dict(D, I, query_ids, self.rev_mapping)

    def retrieve_all_with_emb(self, query_emb, query_ids, min_score=0):
        """Every hit, not the top_k: the query forms of retrieve_with_emb -> {qid: {pid: score}} of ALL documents that share a term with the
        query and score above `min_score` (ImpactIndex.range_search; scores are >= 1, so the default keeps every hit).  A pid indexed twice
        keeps the score of its later row, as in retrieve_with_emb."""
        assert len(query_emb) == len(query_ids)
        csr = self._query_rows(query_emb) if isinstance(query_emb, SparseRows) else query_csr([self._query_terms(q) for q in query_emb])
        lims, D, I = self.impact_index.range_search(*csr, float(min_score))
        lims, D, I = lims.cpu().tolist(), D.cpu().tolist(), I.cpu().tolist()
        rev = self.rev_mapping
        return {qid: {rev[I[j]]: D[j] for j in range(lims[i], lims[i + 1])} for i, qid in enumerate(query_ids)}


class HybridSearch:
    """Dense half of the reference's HybridSearch: routes `dense_reps` -> results["den"], `emb_reps` -> results["emb"]
    (hybrid_search.py:121-180); `search()` returns the last enabled type unless return_all_results."""

    def __init__(self, model, batch_size: int = 128, corpus_chunk_size: Optional[int] = None, use_multiple_gpu: bool = False,
                 score_fuse_method: str = "linear", fuse_weights=(0.7, 0.3), return_all_results: bool = False, sparse_search=None,
                 sparse_format: str = "json", **kwargs):
        """sparse_search: an engine with the reference's AnseriniSearch interface (`index(corpus_emb, corpus_ids)`,
        `retrieve_with_emb(query_emb, query_ids, top_k)`, `_clear()`); the Lucene engine itself is outside this package.  When
        one is given, `tok` / `emb_tok` (query token counts x sparse document vectors, and their fusion with the dense hits,
        hybrid_search.py:160-180) are produced like the reference does; the fusion runs on the GPU (score_fuse_utils).
        sparse_search="gpu": this package's own engine, an ImpactSearch (it gets the anserini_* arguments among **kwargs).
        sparse_format="csr" (with this package's engine only): the model's encode_corpus / encode_queries are called with sparse_format="csr"
        and hand their `sparse_reps` over as SparseRows on the GPU; "json" (default) passes nothing new to the model."""
        self.model = model
        self.score_fuse_method = score_fuse_method
        self.fuse_weights = list(fuse_weights)
        if isinstance(sparse_search, str):
            if sparse_search != "gpu":
                raise ValueError(f"HybridSearch: sparse_search={sparse_search!r} (an engine object, None or 'gpu')")
            sparse_search = ImpactSearch(model, batch_size=batch_size, corpus_chunk_size=corpus_chunk_size,
                                         **{a: kwargs[a] for a in ("anserini_impact_search", "anserini_vector_type") if a in kwargs})
        self.sparse_search = sparse_search
        if sparse_format not in ("json", "csr"):
            raise ValueError(f"HybridSearch: sparse_format={sparse_format!r} ('json' or 'csr')")
        if sparse_format == "csr" and not isinstance(sparse_search, ImpactSearch):
            raise ValueError("HybridSearch: sparse_format='csr' needs this package's sparse engine (sparse_search='gpu' or an ImpactSearch); "
                             f"got {type(sparse_search).__name__}")
        self.sparse_format = sparse_format
        self._encode_kwargs = {"sparse_format": "csr"} if sparse_format == "csr" else {}
        self.batch_size = batch_size
        self.corpus_chunk_size = batch_size * 800 if corpus_chunk_size is None else corpus_chunk_size
        self.show_progress_bar = kwargs.get("show_progress_bar", True)
        self.convert_to_tensor = kwargs.get("convert_to_tensor", True)
        # faiss_search_map (hybrid_search.py:32-70): "flat" (default), "sq" (QT_fp16 / QT_8bit_uniform), "pq" (IndexPQ), "binary" (IndexBinaryFlat + rerank),
        # "pca" (IndexPreTransform(PCAMatrix, base)), "refine" (IndexRefineFlat over a pq / sq / pca / ivfpq / ivfsq base), "ivf" (IndexIVFFlat), "ivfpq"
        # (IndexIVFPQ), "ivfsq" (IndexIVFScalarQuantizer, QT_fp16) and "ivfsq8" (IndexIVFScalarQuantizer, QT_8bit / QT_8bit_uniform) are served;
        # "graph" (HNSWFaissSearch: a fixed-degree graph + beam search over GraphFlatIndex, the native way to the reference's hnsw_* arguments);
        # anything else ("hnsw", "hnswsq") is served flat
        faiss_search_map = kwargs.get("faiss_search_map", "flat")
        den_cls = {"sq": SQFaissSearch, "pq": PQFaissSearch, "binary": BinaryFaissSearch, "pca": PCAFaissSearch,
                   "refine": RefineFaissSearch, "ivf": IVFFaissSearch, "ivfpq": IVFPQFaissSearch, "ivfsq": IVFSQFaissSearch,
                   "ivfsq8": IVFSQ8FaissSearch, "graph": HNSWFaissSearch}.get(faiss_search_map, FlatIPFaissSearch)
        if faiss_search_map not in ("flat", "sq", "pq", "binary", "pca", "refine", "ivf", "ivfpq", "ivfsq", "ivfsq8", "graph"):
            logger.warning("HybridSearch: faiss_search_map=%r is not served; the dense half runs on the flat index (the graph index is "
                           "faiss_search_map='graph')", faiss_search_map)
        # (the reference passes its **kwargs through to the searcher)
        passed = {"pq": ("num_of_centroids", "code_size", "use_rotation", "similarity_metric"), "sq": ("quantizer_type", "similarity_metric"),
                  "binary": ("binary_k", "threshold"), "pca": ("output_dimension", "base_index", "pca_matrix", "eigen_power", "random_rotation"),
                  "ivf": ("nlist", "nprobe", "similarity_metric"),
                  "ivfpq": ("nlist", "nprobe", "num_of_centroids", "code_size", "by_residual", "similarity_metric"),
                  "ivfsq": ("nlist", "nprobe", "quantizer_type", "by_residual", "similarity_metric"),
                  "ivfsq8": ("nlist", "nprobe", "quantizer_type", "by_residual", "similarity_metric"),
                  "graph": ("hnsw_store_n", "hnsw_ef_search", "hnsw_ef_construction", "similarity_metric")}
        den_kwargs = {a: kwargs[a] for a in passed.get(faiss_search_map, ()) if a in kwargs}
        if faiss_search_map == "pca" and kwargs.get("output_dimension") is None:
            raise ValueError("HybridSearch: faiss_search_map='pca' needs output_dimension (the dimension after the PCA)")
        if faiss_search_map == "refine":              # its own arguments and those of the base searcher it names
            names = ("refine_base", "k_factor", "refine_type") + passed.get(kwargs.get("refine_base"), ())
            den_kwargs = {a: kwargs[a] for a in names if a in kwargs}
        self.dense_search = den_cls(model, batch_size=batch_size, corpus_chunk_size=corpus_chunk_size, use_multiple_gpu=use_multiple_gpu, **den_kwargs)
        self.dense_search.encode_kwargs = dict(self._encode_kwargs)
        self.return_all_results = return_all_results
        self.mteb_model_meta = None

    @classmethod
    def name(cls):
        return "hybrid_search"

    def encode(self, sentences, batch_size, **kw):
        return self.model.encode(sentences=sentences, batch_size=batch_size, **kw)

    def encode_queries(self, queries, batch_size, **kw):
        return self.model.encode_queries(queries=queries, batch_size=batch_size, **{**self._encode_kwargs, **kw})

    def encode_corpus(self, corpus, batch_size, **kw):
        return self.model.encode_corpus(corpus=corpus, batch_size=batch_size, **{**self._encode_kwargs, **kw})

    def _clear(self, dense: bool = True, sparse: bool = True):
        if dense:
            self.dense_search._clear()
        if sparse and self.sparse_search is not None:
            self.sparse_search._clear()

    def index(self, corpus_emb: dict, corpus_ids: list):
        assert isinstance(corpus_emb, dict) and corpus_emb.get("dense_reps") is not None
        self.dense_search.index(corpus_emb["dense_reps"], corpus_ids)
        if self.sparse_search is not None and corpus_emb.get("sparse_reps") is not None:
            self.sparse_search.index(corpus_emb["sparse_reps"], corpus_ids)

    def _fuse_results(self, dense_results=None, sparse_results=None, weights=(0.7, 0.3)):
        """hybrid_search.py:207-232: one of the lists alone, or their RRF / min-max linear fusion (on the GPU)."""
        from .score_fuse_utils import fuse_scores_linear, fuse_scores_rrf
        if dense_results is None and sparse_results is None:
            raise ValueError("All scores are None. Please check model settings.")
        if dense_results is None:
            return sparse_results
        if sparse_results is None:
            return dense_results
        if self.score_fuse_method == "rrf":
            return fuse_scores_rrf([dense_results, sparse_results])
        if self.score_fuse_method == "linear":
            return fuse_scores_linear([dense_results, sparse_results], weights=weights)
        raise NotImplementedError(f"score_fuse_method {self.score_fuse_method} is not supported.")

    def retrieve_with_emb(self, query_emb: dict, query_ids: list, top_k: int, dense: bool = True, sparse: bool = True, **kwargs):
        assert isinstance(query_emb, dict) and (query_emb.get("dense_reps") is not None or query_emb.get("emb_reps") is not None)
        results = {}
        if dense:
            if query_emb.get("dense_reps") is not None:
                results["den"] = self.dense_search.retrieve_with_emb(query_emb["dense_reps"], query_ids, top_k=top_k)
            if query_emb.get("emb_reps") is not None:
                results["emb"] = self.dense_search.retrieve_with_emb(query_emb["emb_reps"], query_ids, top_k=top_k)
        if sparse and self.sparse_search is not None and query_emb.get("token_id_reps") is not None:
            results["tok"] = self.sparse_search.retrieve_with_emb(query_emb["token_id_reps"], query_ids, top_k=top_k)
        if sparse and self.sparse_search is not None and query_emb.get("sparse_reps") is not None:       # LM-head sparse queries (hybrid_search.py:166-172)
            results["spr"] = self.sparse_search.retrieve_with_emb(query_emb["sparse_reps"], query_ids, top_k=top_k)
            if "den" in results:
                results["den_spr"] = self._fuse_results(results["den"], results["spr"], weights=self.fuse_weights)
        if "emb" in results and "tok" in results:
            results["emb_tok"] = self._fuse_results(results["emb"], results["tok"], weights=self.fuse_weights)
        return results

    def search(self, corpus, queries, top_k: int = 1000, score_function: str = None, return_sorted: bool = False,
               ignore_identical_ids: bool = False, **kwargs):
        query_ids, queries_list = _ids_and_list(queries)
        qe = self.model.encode_queries(queries_list, batch_size=self.batch_size, show_progress_bar=self.show_progress_bar,
                                       convert_to_tensor=self.convert_to_tensor, **self._encode_kwargs)
        assert isinstance(qe, dict) and any(k in qe for k in ("dense_reps", "emb_reps", "sparse_reps", "token_id_reps"))
        results, default = {}, None
        # one corpus pass serves every enabled query representation (they share the document `dense_reps`)
        kinds = [(k, name) for k, name in (("dense_reps", "den"), ("emb_reps", "emb")) if qe.get(k) is not None]
        # sparse half (hybrid_search.py:330-375): every chunk's document vectors go into the engine as they are encoded, the engine is
        # searched once at the end with the queries' token-id counts, `emb_tok` is the fusion of the two final hit lists
        use_tok = self.sparse_search is not None and qe.get("token_id_reps") is not None
        use_spr = self.sparse_search is not None and qe.get("sparse_reps") is not None      # LM-head sparse query vectors (pseudo text), hybrid_search.py:364-369
        on_chunk = None
        if use_tok or use_spr:
            def on_chunk(chunk_ids, enc):
                assert enc.get("sparse_reps") is not None, "sparse engine given but encode_corpus returned no sparse_reps"
                self.sparse_search.index(enc["sparse_reps"], list(chunk_ids))
        multi = _chunked_dense_search(self.dense_search, [qe[k] for k, _ in kinds], query_ids, corpus, top_k, ignore_identical_ids, on_chunk=on_chunk)
        dense_res = dict(zip([name for _, name in kinds], multi))
        tok_res = self.sparse_search.retrieve_with_emb(query_emb=qe["token_id_reps"], query_ids=query_ids, top_k=top_k) if use_tok else None
        spr_res = self.sparse_search.retrieve_with_emb(query_emb=qe["sparse_reps"], query_ids=query_ids, top_k=top_k) if use_spr else None
        # result names and the default (the LAST one set) in the reference's order (hybrid_search.py:380-403): den, spr, emb, tok, den_spr, emb_tok
        if "den" in dense_res:
            results["den"] = default = dense_res["den"]
        if use_spr:
            results["spr"] = default = spr_res
        if "emb" in dense_res:
            results["emb"] = default = dense_res["emb"]
        if use_tok:
            results["tok"] = default = tok_res
        if "den" in dense_res and use_spr:
            results["den_spr"] = default = self._fuse_results(dense_res["den"], spr_res, weights=self.fuse_weights)
        if "emb" in dense_res and use_tok:
            results["emb_tok"] = default = self._fuse_results(dense_res["emb"], tok_res, weights=self.fuse_weights)
        self._clear()
        return results if self.return_all_results else default


# ------------------------------------------------------------------------------------------------------------------
def _as_device(x, device):
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=torch.float32).contiguous()


def _to_result_dict(scores: torch.Tensor, ids: torch.Tensor, query_ids: list, rev_mapping) -> dict:
    """[Q, k] device arrays -> {qid: {pid: score}} (retriever/faiss_search.py:165-171, hybrid_search.py:347-355).  rev_mapping: row -> pid as a
    dict or a sequence (empty / None: the row number as a string).  One D2H copy, then per query an object-array gather of the pids and
    dict(zip(...)) over Python lists -- no per-hit Python arithmetic (1000 queries x top-1000: 0.21 s instead of 0.79 s; the nested dict is
    the reference's return type)."""
    S, I = scores.cpu().numpy(), ids.cpu().numpy()
    names = None
    if rev_mapping is not None and len(rev_mapping):
        if isinstance(rev_mapping, dict):
            names = np.empty(max(rev_mapping) + 1, dtype=object)
            names[list(rev_mapping.keys())] = list(rev_mapping.values())
        else:
            names = np.empty(len(rev_mapping), dtype=object)
            names[:] = list(rev_mapping)
    out = {}
    for qi, qid in enumerate(query_ids):
        r, sc = I[qi], S[qi]
        keep = r >= 0
        if not keep.all():
            r, sc = r[keep], sc[keep]
        keys = names[r].tolist() if names is not None else [str(x) for x in r.tolist()]
        out[qid] = dict(zip(keys, sc.tolist()))
    return out


def _chunked_dense_search(searcher: FlatIPFaissSearch, query_embs, query_ids: list, corpus, top_k: int, ignore_identical_ids: bool,
                          on_chunk=None):
    """Chunk loop of faiss_search.py:228-291 / hybrid_search.py:301-358: encode chunk -> index -> retrieve -> merge.
    `query_embs` may be one tensor or a list of tensors (several query representations scored against the same docs).
    `on_chunk(corpus_ids_of_chunk, encode_corpus_result)`: called after each chunk is encoded (the sparse half of
    HybridSearch.index, hybrid_search.py:330-331); single-process launch only."""
    single = not isinstance(query_embs, (list, tuple))
    qlist = [query_embs] if single else list(query_embs)
    corpus_ids, docs = _sorted_corpus(corpus)
    n = len(docs)
    device = searcher.model.model.device if hasattr(searcher.model, "model") and hasattr(searcher.model.model, "device") else torch.device("cuda", torch.cuda.current_device())
    qlist = [_as_device(q, device) for q in qlist]
    dim = qlist[0].shape[1]
    Q = len(query_ids)
    row_of = {c: i for i, c in enumerate(corpus_ids)}
    ident = torch.tensor([row_of.get(q, -2) for q in query_ids], dtype=torch.int64, device=device) if ignore_identical_ids else None
    run_D = [torch.full((Q, top_k), -FLT_MAX, dtype=torch.float32, device=device) for _ in qlist]
    run_I = [torch.full((Q, top_k), -1, dtype=torch.int64, device=device) for _ in qlist]
    # cross-chunk ties (hybrid_search.py:182-205: heapq on (score, pid) tuples keeps the larger pid): the running list carries
    # key = position of the document in DESCENDING pid order, so the merge's (score desc, key asc) is the heap's order
    key_of_row = row_of_key = None
    if n > searcher.corpus_chunk_size:
        try:
            order = sorted(range(n), key=corpus_ids.__getitem__, reverse=True)
        except TypeError:                             # ids of mixed types do not compare (the reference's heap would raise on a tie)
            order = None
        if order is not None:
            row_of_key = torch.tensor(order, dtype=torch.int64, device=device)
            key_of_row = torch.empty_like(row_of_key)
            key_of_row[row_of_key] = torch.arange(n, dtype=torch.int64, device=device)
    rank, world = DenseRetrievalFaissSearch._rank_world()
    if world > 1:
        from .sharded import exchange_merge, local_to_global_rows
        if on_chunk is not None:
            raise NotImplementedError("a sparse engine needs the chunk's sparse vectors on the calling rank: single-process launch only")
    # the reference's own launch (eval/eval_utils.py: torch RPC, only rank 0 drives): shards live on the RPC workers
    rpc_names = []
    if world == 1:
        from . import rpc_shards
        rpc_names = rpc_shards.rpc_workers()
        if len(rpc_names) <= 1 or "model" not in rpc_shards._WORKER or on_chunk is not None:
            rpc_names = []                            # (with a sparse engine the calling rank encodes everything itself)
        elif not getattr(searcher, "serves_rpc_shards", True):
            raise NotImplementedError(f"{type(searcher).__name__}: shards on RPC workers are not served (rpc_shards builds flat shards); "
                                      "use a single-process or one-process-per-GPU launch")
    for s in range(0, n, searcher.corpus_chunk_size):
        e = min(s + searcher.corpus_chunk_size, n)
        logger.info("Encoding Batch %d/%d...", s // searcher.corpus_chunk_size + 1, -(-n // searcher.corpus_chunk_size))
        if world > 1:
            # one process per GPU: batch j of this chunk's sorted documents belongs to rank j % world; every rank
            # encodes its batches into its own HBM shard whose rows carry their global sorted position
            rows = (local_to_global_rows(e - s, searcher.batch_size, rank, world) + s).tolist()
            searcher._index_in_place([docs[i] for i in rows], rows, dim)
        elif rpc_names:
            rpc_shards.index_chunk(rpc_names, docs[s:e], s, dim, searcher.batch_size)   # texts out, nothing back
        else:
            enc = searcher._index_in_place(docs[s:e], list(range(s, e)), dim)   # rows carry their global sorted position
            if on_chunk is not None and enc is not None:
                on_chunk(corpus_ids[s:e], enc)
        for j, q in enumerate(qlist):
            if rpc_names:                             # local top-k of every worker's shard (Q x k pairs each), merged here
                D, I = merge_topk(*rpc_shards.search_shards(rpc_names, q, top_k, searcher.batch_size))
            else:
                D, I = searcher._retrieve_device(q, top_k)
            if world > 1:                             # one all-gather of the packed per-shard lists, merge on every rank
                D, I = exchange_merge(D, I)
            if ident is not None:                     # drop the qid == pid hit AFTER the per-chunk top_k, like the reference
                hit = I == ident[:, None]
                D = torch.where(hit, torch.full_like(D, -FLT_MAX), D)
                I = torch.where(hit, torch.full_like(I, -1), I)
            if key_of_row is not None:
                I = torch.where(I >= 0, key_of_row[I.clamp(min=0)], I)
            run_D[j], run_I[j] = merge_topk(torch.stack([run_D[j], D]), torch.stack([run_I[j], I]))
        if rpc_names:
            rpc_shards.clear_shards(rpc_names, searcher.batch_size)
        searcher._clear()
    if row_of_key is not None:
        run_I = [torch.where(i >= 0, row_of_key[i.clamp(min=0)], i) for i in run_I]
    outs = [_to_result_dict(d, i, query_ids, corpus_ids) for d, i in zip(run_D, run_I)]
    return outs[0] if single else outs
