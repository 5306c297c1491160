from lightretriever_amd.retriever import BinaryFaissSearch, DenseRetrievalFaissSearch, FlatIPFaissSearch, PCAFaissSearch, PQFaissSearch, RefineFaissSearch, SQFaissSearch  # noqa: F401
