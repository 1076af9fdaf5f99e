"""numpy restatement of the frame statistics (include/vkr_frame_statistics.h, csrc/frame_statistics.hip).

The kernels are pinned against these functions bit for bit; tests/test_frame_statistics.py pins these functions
against exact rational arithmetic.  Everything is IEEE binary64, one rounding per operation, in the order the
header gives."""
import numpy as np

BLOCK = 256  # pixels per block of the error sums


def reference_accumulate(frames, sums=None, squares=None):
    """S and Q of include/vkr_frame_statistics.h for `frames` (an iterable of float32 arrays (..., 4) or (..., 3),
    alpha ignored) in the order given, continued from `sums` / `squares` if given.  Returns (S, Q) as float64
    arrays (pixels, 3)."""
    for frame in frames:
        x = np.asarray(frame, np.float32)
        x = x.reshape(-1, x.shape[-1])[:, :3].astype(np.float64)
        if sums is None:
            sums, squares = np.zeros_like(x), np.zeros_like(x)
        with np.errstate(all="ignore"):
            sums = sums + x
            # (the product of two floats is exact in binary64)
            squares = squares + x * x
    return sums, squares


def reference_mean_variance(sums, squares, frame_count):
    """(mean, variance) as float32 arrays (pixels, 4) with alpha 1; variance is None for fewer than two frames,
    which resolve_frame_statistics() refuses"""
    if frame_count < 1:
        raise ValueError("no frame was accumulated")
    sums, squares = np.asarray(sums, np.float64), np.asarray(squares, np.float64)
    n = np.float64(frame_count)

    def rgba(values):
        out = np.ones(values.shape[:-1] + (4,), np.float32)
        with np.errstate(all="ignore"):
            out[..., :3] = values.astype(np.float32)
        return out
    with np.errstate(all="ignore"):
        mean = rgba(sums / n)
        if frame_count < 2:
            return mean, None
        v = (squares - (sums * sums) / n) / np.float64(frame_count - 1)
        # (NaN and -0 fail the comparison and pass through)
        v = np.where(v < 0, np.float64(0), v)
    return mean, rgba(v)


def reference_tree_sum(terms):
    """The error sums' order of additions for float64 `terms` of shape (count,) or (count, channels): blocks of 256
    slots padded with +0.0, halved by slot[j] += slot[j + s] for s = 128 ... 1, then the blocks' partials added in block
    order from +0.0.  Returns a float64 scalar or (channels,) array."""
    e = np.asarray(terms, np.float64)
    flat = e.ndim == 1
    e = e.reshape(len(e), -1)
    blocks = max((len(e) + BLOCK - 1) // BLOCK, 1)
    p = np.zeros((blocks * BLOCK, e.shape[1]), np.float64)
    p[:len(e)] = e
    p = p.reshape(blocks, BLOCK, -1)
    with np.errstate(all="ignore"):
        while p.shape[1] > 1:
            h = p.shape[1] // 2
            p = p[:, :h] + p[:, h:]
        total = np.zeros(e.shape[1], np.float64)
        for partial in p[:, 0]:
            total = total + partial
    return total[0] if flat else total


def squared_difference_terms(a, b):
    """The terms of sum_squared_differences() for two float32 arrays (..., >= 3): (pixels, 3) float64"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        d = a.reshape(-1, a.shape[-1])[:, :3].astype(np.float64) - b.reshape(-1, b.shape[-1])[:, :3].astype(np.float64)
        return d * d


def frame_terms(a):
    """The terms of sum_frame(): (pixels, 3) float64"""
    a = np.asarray(a, np.float32)
    return a.reshape(-1, a.shape[-1])[:, :3].astype(np.float64)
