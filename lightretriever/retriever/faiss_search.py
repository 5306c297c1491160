from lightretriever_amd.retriever import DenseRetrievalFaissSearch, FlatIPFaissSearch, PQFaissSearch, SQFaissSearch  # noqa: F401
