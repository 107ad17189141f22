"""Solver families ("models"): CPU oracle, scalar pair path, MFMA block path,
and the batched path for many small matrices.

The distributed block solver lives in ``parallel.distributed``.
"""
from .base import BatchedSVDResult, SVDResult, Solver  # noqa: F401
from .batched import BatchedJacobi  # noqa: F401
from .block import BlockJacobi  # noqa: F401
from .oracle import OracleJacobi  # noqa: F401
from .scalar import ScalarJacobi  # noqa: F401
