from lightretriever_amd.retriever import BinaryFaissSearch, DenseRetrievalFaissSearch, FlatIPFaissSearch, PCAFaissSearch, PQFaissSearch, SQFaissSearch  # noqa: F401
