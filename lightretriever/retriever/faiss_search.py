from lightretriever_amd.retriever import BinaryFaissSearch, DenseRetrievalFaissSearch, FlatIPFaissSearch, IVFFaissSearch, PCAFaissSearch, PQFaissSearch, RefineFaissSearch, SQFaissSearch  # noqa: F401
