"""What the built octrees of ``ops.winding`` and ``ops.icp`` share (csrc/octree_common.h): views of one device buffer that holds B trees
of one stride, every array at one offset in all of them; and ``_ws``, the workspace allocation of the launchers around them."""
import torch

from ._base import I32


def _ws(nbytes, dev):
    return torch.empty((max(int(nbytes), 8) + 7) // 8, dtype=torch.int64, device=dev)


class _Octree:
    """``buf`` (int64 device buffer), ``depth``, ``_offsets`` (the layout call's: pyramids, records, list offsets, lists, payloads),
    ``_stride`` (bytes from one problem's tree to the next), ``_items`` (per problem) and ``_leaves`` (occupied leaves per problem)."""

    def _view(self, at, dtype, numel, b=0):
        size = torch.empty((), dtype=dtype).element_size()
        at += b * self._stride
        return self.buf.view(torch.uint8)[at:at + numel * size].view(dtype)

    def _pyramid(self, level, b=0):
        """int32 [8^level]: the rank of an occupied cell among its level's occupied cells in Morton order, or -1."""
        return self._view(self._offsets[0] + 4 * ((8 ** level - 1) // 7), I32, 8 ** level, b)

    def _frame(self, b=0):
        """float64 [4]: the minimum corner and the side."""
        return self._view(0, torch.float64, 4, b)

    def _list_offsets(self, b=0):
        return self._view(self._offsets[2], I32, self._leaves[b] + 1, b)

    def _lists(self, b=0):
        """int32 [items]: the leaves' item indices, leaf after leaf in Morton order, ascending inside a leaf."""
        return self._view(self._offsets[3], I32, self._items, b)
