"""Oracle: the counter-based dropout draw, restated in plain numpy (TEST INFRASTRUCTURE, see oracle/__init__.py).

The specification of the draw the HIP kernels make in place ("The dropout draw"); nothing of the package under test
is imported here.  Element ``idx`` of the dense [M, C] (NHWC) tensor, idx = m * C + c whatever the pitch or the base pointer of
the operand, is kept when

    float32(u24(seed, idx)) * float32(2^-24) >= float32(p)

and a kept element is multiplied by ``keep_scale(p)`` in one fp32 product.  All integer arithmetic is uint64 and wraps."""
import numpy as np

G = 0x9E3779B97F4A7C15            # the seed multiplier: the masks of two seeds are windows of one sequence, s * G apart
_M1, _M2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
_MASK64 = (1 << 64) - 1


def _indices(idx):
    return np.ascontiguousarray(idx, dtype=np.uint64)


def u24(seed, idx):
    """the 24 random bits of element ``idx`` (an integer or an array of them) under ``seed``: the murmur3 64-bit finaliser of
    seed * G + idx, low 32 bits, top 24 of those"""
    base = np.uint64((int(seed) * G) & _MASK64)
    with np.errstate(over="ignore"):
        x = _indices(idx) + base
        x ^= x >> np.uint64(33)
        x *= np.uint64(_M1)
        x ^= x >> np.uint64(33)
        x *= np.uint64(_M2)
        x ^= x >> np.uint64(33)
    return ((x & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.uint32)


def uniform01(seed, idx):
    """u24 / 2^24 as the fp32 value the kernels compare with p (exact: 24 bits fit the significand)"""
    return u24(seed, idx).astype(np.float32) * np.float32(2.0 ** -24)


def keep(seed, n_or_shape, p, start=0):
    """bool keep mask of the elements start .. start + n in logical order, shaped like ``n_or_shape`` (an element count, or the
    dense shape whose C order is the logical index: [M, C], [B, H, W, C])"""
    shape = (int(n_or_shape),) if np.isscalar(n_or_shape) else tuple(int(s) for s in n_or_shape)
    n = int(np.prod(shape, dtype=np.int64))
    idx = np.arange(start, start + n, dtype=np.uint64)
    return (uniform01(seed, idx) >= np.float32(p)).reshape(shape)


def keep_scale(p):
    """1 / (1 - p) as the kernels form it: fp32 subtraction, fp32 division"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def window_offsets(seeds):
    return np.array([(int(s) * G) & _MASK64 for s in seeds], dtype=np.uint64)


def window_gap(seeds):
    """the smallest distance mod 2^64 between the window offsets s * G of a set of seeds (a Python int; 0 when a seed repeats).
    Two masks of N elements each are disjoint windows of the sequence exactly while the gap of their seeds is at least N."""
    off = np.sort(window_offsets(seeds))
    if off.size < 2:
        return 1 << 64
    with np.errstate(over="ignore"):
        d = np.diff(off)
        wrap = off[0] - off[-1]                     # uint64 wrap-around: the distance across 2^64
    return int(min(int(d.min()), int(wrap)))


def shift_distance(k):
    """|k * G mod 2^64| as a distance: how far apart the windows of two seeds that differ by k lie (k an int or an array)"""
    with np.errstate(over="ignore"):
        d = _indices(k) * np.uint64(G)
        return np.minimum(d, np.uint64(0) - d)
