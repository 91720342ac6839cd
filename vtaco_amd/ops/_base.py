"""What every kernel family shares: the library handle, pointer helpers and hipGraph keep-alive."""
import ctypes

import torch

from .. import _lib
from .._lib import VtError, check, dev_ptr, stream_ptr


I32 = torch.int32
U8 = torch.uint8


# ---- hipGraph capture support -------------------------------------------------------------------------------------
# A captured graph holds RAW POINTERS to everything its launches read: derived buffers (packed weights, the decoder
# blob, the UNet3D workspace) live in caches that re-allocate when a weight changes or another shape runs.  While a
# capture is being prepared every launcher hands such tensors to ``keep_for_graph``; the graph's owner stores the list
# next to the graph, so the memory cannot be recycled under a live graph.
_graph_keep = None


class graph_keepalive:
    """``with ops.graph_keepalive() as keep:`` -- collects every derived tensor the launchers inside touch."""

    def __enter__(self):
        global _graph_keep
        self._prev, _graph_keep = _graph_keep, []
        return _graph_keep

    def __exit__(self, *exc):
        global _graph_keep
        _graph_keep = self._prev
        return False


def keep_for_graph(*tensors):
    if _graph_keep is not None:
        _graph_keep.extend(t for t in tensors if t is not None)


def _c(t):
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


def _ptr_array(tensors, name):
    """A host array of device pointers (ctypes c_void_p * K) for the K int32 tensors, or None entries."""
    arr = (ctypes.c_void_p * len(tensors))()
    for k, t in enumerate(tensors):
        arr[k] = dev_ptr(t, name, I32).value if t is not None else None
    return arr
