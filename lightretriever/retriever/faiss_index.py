from lightretriever_amd.retriever import FaissBinaryIndex, FaissHNSWIndex, FaissIndex  # noqa: F401
