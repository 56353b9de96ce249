"""parallel_hnsw_amd: MI355X-native HNSW build + search behind the public surface of the
Rust crate terminusdb-labs/parallel-hnsw (hot path only)."""
from ._lib import BuildParams, OptimizationParams, PhnswError, SearchParams, build_lib, lib  # noqa: F401
from .hnsw import (ATTR_NONE, Attribute, LabeledAttribute, attr_keys, EMPTY, FILTER_ALL, LABEL_NONE, Labels, METRIC_COSINE_HALF, METRIC_L2, METRIC_ONE_MINUS_DOT, BuildParameters,  # noqa: F401
                   Hnsw, Layer,
                   SearchParameters, Stored, Unstored, VectorStore, PqStore, SharedPqStore, F16Store, I8Store, I8QStore, BitStore,
                   QuantizedHnsw, stream_create_beside)
from .sharded import (EmulatedComm, GpuEngine, PythonEngine, ShardedBuilder, TorchComm, build_sharded,  # noqa: F401,E402
                      improve_index_sharded, sharded_tuning)
