from lightretriever_amd.retriever import BinaryFaissSearch, DenseRetrievalFaissSearch, FlatIPFaissSearch, PQFaissSearch, SQFaissSearch  # noqa: F401
