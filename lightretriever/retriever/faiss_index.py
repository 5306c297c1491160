from lightretriever_amd.retriever import FaissBinaryIndex, FaissIndex  # noqa: F401
