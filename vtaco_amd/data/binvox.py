"""Reader and writer of the binvox voxel format (https://www.patrickmin.com/binvox/binvox.html), written from the format's description.

A file is an ASCII header -- ``#binvox 1``, ``dim d0 d1 d2``, ``translate tx ty tz``, ``scale s``, ``data`` -- followed by run-length
pairs of bytes (value, count) that cover d0 * d1 * d2 voxels.  The voxels are stored with the y index running fastest and the z index
next, so the array reshaped to ``dim`` is indexed [x][z][y]; ``read_as_3d_array`` hands back [x][y][z] and ``write`` takes [x][y][z]."""
from __future__ import annotations

import numpy as np


class Voxels:
    """``data`` bool [d0,d1,d2] (after the axis swap: [x][y][z]), ``dims``, ``translate``, ``scale`` as the header gives them."""

    def __init__(self, data, dims, translate, scale):
        self.data, self.dims, self.translate, self.scale = data, dims, translate, scale


def read_header(fp):
    """(dims, translate, scale); leaves ``fp`` at the first byte of the run-length data."""
    magic = fp.readline().strip()
    if not magic.startswith(b'#binvox'):
        raise IOError('not a binvox file (first line %r)' % magic[:16])
    dims, translate, scale = None, [0.0, 0.0, 0.0], 1.0
    while True:
        line = fp.readline()
        if not line:
            raise IOError('binvox header ends without a data line')
        words = line.strip().split()
        if not words:
            continue
        if words[0] == b'data':
            break
        if words[0] == b'dim':
            dims = [int(w) for w in words[1:4]]
        elif words[0] == b'translate':
            translate = [float(w) for w in words[1:4]]
        elif words[0] == b'scale':
            scale = float(words[1])
    if dims is None or len(dims) != 3 or min(dims) < 1:
        raise IOError('binvox header has no usable dim line')
    return dims, translate, scale


def read_as_3d_array(fp, fix_coords=True):
    """The dense occupancy array of an open binary file.  ``fix_coords``: swap the last two axes so that the result is indexed
    [x][y][z] (the storage order is [x][z][y])."""
    dims, translate, scale = read_header(fp)
    raw = np.frombuffer(fp.read(), dtype=np.uint8)
    if raw.size % 2:
        raise IOError('binvox run-length data has an odd number of bytes')
    values, counts = raw[0::2], raw[1::2]
    total = dims[0] * dims[1] * dims[2]
    if int(counts.sum(dtype=np.int64)) != total:
        raise IOError('binvox run lengths cover %d voxels, the header says %d' % (int(counts.sum(dtype=np.int64)), total))
    data = np.repeat(values, counts).astype(bool).reshape(dims)
    if fix_coords:
        data = np.transpose(data, (0, 2, 1))
    return Voxels(data, dims, translate, scale)


def write(voxels, fp):
    """Write a ``Voxels`` (``data`` bool [x][y][z]) to an open binary file in the run-length format above: the header lines with
    ``str`` of the numbers, then (value, count) byte pairs over the voxels in [x][z][y] order, a run ending at 255 voxels."""
    data = np.asarray(voxels.data).astype(bool)
    if data.ndim != 3:
        raise ValueError('binvox.write: data must be a 3-D array')
    head = '#binvox 1\ndim %s\ntranslate %s\nscale %s\ndata\n' % (
        ' '.join(str(int(d)) for d in voxels.dims), ' '.join(str(t) for t in voxels.translate), str(voxels.scale))
    fp.write(head.encode('ascii'))
    flat = np.transpose(data, (0, 2, 1)).reshape(-1).astype(np.uint8)
    if flat.size == 0:
        return
    starts = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1])
    lengths = np.diff(np.concatenate([starts, [flat.size]]))
    values = flat[starts]
    # a run of n voxels: n // 255 pairs of 255, then the remainder; like the reference's writer, a run that is followed by another one
    # always ends with its remainder pair, even when that is (value, 0) -- readers repeat it zero times
    full, rest = lengths // 255, lengths % 255
    tail = rest > 0
    tail[:-1] = True
    pairs = full + tail
    out_v = np.repeat(values, pairs)
    out_c = np.full(out_v.size, 255, dtype=np.uint8)
    ends = np.cumsum(pairs) - 1
    out_c[ends[tail]] = rest[tail]
    fp.write(np.stack([out_v, out_c], axis=1).astype(np.uint8).tobytes())
