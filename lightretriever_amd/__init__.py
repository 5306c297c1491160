"""lightretriever_amd: MI355X-native corpus-embedding + flat-IP search path of LightRetriever."""
from .encoder import EncoderConfig, LrxEncoder, interleave_gate_up, lora_merge, rope_tables  # noqa: F401
from .index import BinaryFlatIndex, FlatIPIndex, PQIndex, SQ8Index, SQFp16Index, merge_topk  # noqa: F401
from .impact_index import ImpactIndex  # noqa: F401
from .sparse_rows import SparseRows  # noqa: F401
from .transform import PCAMatrix, PreTransformIndex  # noqa: F401
from .refine import RefineFlatIndex  # noqa: F401
from .graph import GraphFlatIndex  # noqa: F401
from .ivf import IVFFlatIndex  # noqa: F401
from .selector import RowSelector  # noqa: F401
from .ivfpq import IVFPQIndex  # noqa: F401
from .ivfsq import IVFSQIndex  # noqa: F401
from .ivfsq8 import IVFSQ8Index  # noqa: F401
