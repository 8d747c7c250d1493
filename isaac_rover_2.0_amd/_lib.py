"""ctypes binding of librover_step.so (C ABI in include/rover_step.h): the public face.  ``_abi`` mirrors the header and holds the loader and
the checked call paths; ``_core``, ``_scene``, ``_sim`` and ``_learn`` hold the entry points of one C unit each.  Every name of theirs is
importable from here: the star imports carry the public ones, the lists below the private ones that callers and tests use.

There is NO CPU fallback: if the HIP library is missing or a call fails, this module raises.  Tensors are PyTorch-ROCm tensors; only their
``data_ptr()`` crosses the boundary, and work is enqueued on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

from ._abi import *
from ._abi import _CSRC, _FAKE, _P, _host, _lib, _ptr, _raw_stream, _rows, _sources, _stream
from ._core import *
from ._learn import *
from ._learn import _precision_suffix
from ._scene import *
from ._sim import *


class Engine(CoreEngine, SceneEngine, SimEngine, LearnEngine):
    """One rover_ctx: owns the device tables, launches the step kernels on torch's current stream."""
