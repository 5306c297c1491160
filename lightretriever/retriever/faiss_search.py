from lightretriever_amd.retriever import DenseRetrievalFaissSearch, FlatIPFaissSearch, SQFaissSearch  # noqa: F401
