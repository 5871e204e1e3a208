"""The independent definition of the input standardisation (include/bsig_input_norm.h) and the case tables of
its tests: numpy, two passes, in np.longdouble; the flat rule written out from the header's text.  Nothing here
knows about slabs, Welford or Chan -- except SLAB, which only picks row counts around the kernel's slab."""
import functools

import numpy as np

SLAB = 64                                                   # BSIG_INPUT_NORM_SLAB_ROWS
N_CASES = (1, 2, SLAB - 1, SLAB, SLAB + 1, 800, 3 * SLAB + 5)
WIDTH_CASES = (1, 3, 4, 5, 255, 256, 257, 1030)             # around the 16-byte group and the 256-thread tile
PITCH_CASES = ('tight', 'aligned', 'odd')
U53 = 2.0 ** -53                                            # a double rounding: the unit of the Welford bounds


def unit_roundoff(dtype):
    """u of the header: 2^-23 for fp32 rows, 2^-52 for double rows."""
    return {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}[np.dtype(dtype)]


def pitch(kind, width, dtype):
    """Row pitch in elements: equal to the width; the width rounded up to 16 bytes; an odd pitch above the
    width, whose rows cannot all be 16-byte aligned (the element-by-element path)."""
    per16 = 16 // np.dtype(dtype).itemsize
    return {'tight': width, 'aligned': -(-width // per16) * per16, 'odd': (width + 1) | 1}[kind]


def reference_stats(x):
    """(mean, std, flat) of the columns of x[n, width] by the header's definition: two passes in long double,
    the population standard deviation, flat when std <= 8 u |mean|.  mean and std are long doubles."""
    xl = np.asarray(x).astype(np.longdouble)
    n = xl.shape[0]
    mean = xl.sum(axis=0) / n
    dev = xl - mean
    std = np.sqrt((dev * dev).sum(axis=0) / n)
    flat = std <= 8 * np.longdouble(unit_roundoff(x.dtype)) * np.abs(mean)
    return mean, std, flat


def reference_inv_std(std, flat):
    """inv_std of the header as float64: 0 for a flat column, else 1 / std."""
    return np.where(flat, 0.0, 1.0 / np.where(flat, 1.0, std.astype(np.float64)))


def apply(x, mean, inv_std):
    """The header's apply step: widen, ONE double subtraction, ONE double multiplication, round once."""
    x = np.asarray(x)
    return ((x.astype(np.float64) - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64)).astype(x.dtype)


def standardize(x, n_stats=None):
    """x standardised by the long-double statistics of its first n_stats rows (default: all), through
    float64 mean / inv_std and the header's apply step; in x's own type."""
    mean, std, flat = reference_stats(x[:n_stats])
    return apply(x, mean.astype(np.float64), reference_inv_std(std, flat))


# ---- the columns of the statistics tests, by column index modulo len(COLUMN_KINDS)
# 'far': mean 1e6.  In double rows with std 1, |mean| / std = 1e6 (the one-pass sum-of-squares formula loses four
# digits there).  In fp32 rows the flat threshold at that mean is 8 * 2^-23 * 1e6 = 0.954, so a std of 1 would sit
# ON the threshold -- which these tests must stay a factor 2 away from, on either side -- and the column is
# drawn with std 4 instead: |mean| / std = 2.5e5, a factor 4.2 inside the kept side.
COLUMN_KINDS = ('normal', 'far', 'constant', 'zero', 'outlier', 'ulps_flat', 'ulps_kept')


@functools.lru_cache(maxsize=None)
def rows(n, width, dtype):
    """x[n, width] of ``dtype`` ('float32' | 'float64') with the column kinds above, in turn."""
    dtype = np.dtype(dtype)
    rng = np.random.RandomState(1000 * n + width)
    x = np.empty((n, width), dtype)
    ulp = np.spacing(dtype.type(1000))
    for j in range(width):
        kind = COLUMN_KINDS[j % len(COLUMN_KINDS)]
        if kind == 'normal':
            col = rng.randn(n)
        elif kind == 'far':
            # (a handful of rows: an even spread of the same scale, so that the sample's std cannot land on
            # the threshold by chance)
            spread = rng.randn(n) if n >= 8 else np.sqrt(3.0) * np.linspace(-1.0, 1.0, n)
            col = 1e6 + spread * (4.0 if dtype == np.float32 else 1.0)
        elif kind == 'constant':
            col = np.full(n, -7.3 + j)
        elif kind == 'zero':
            col = np.zeros(n)
        elif kind == 'outlier':
            col = rng.randn(n)
            col[n // 2] = 1e4
        else:
            # a spread of a few ulps around 1000: k in -2..2 is flat, k in -64..64 is kept (n >= 2)
            k = 2 if kind == 'ulps_flat' else 64
            col = dtype.type(1000) + np.round(np.linspace(-k, k, n)).astype(dtype) * ulp if n > 1 else \
                np.full(n, 1000.0)
        x[:, j] = col.astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n, width, dtype):
    """reference_stats of rows(n, width, dtype), once."""
    return reference_stats(rows(n, width, dtype))


def clear_of_the_threshold(x, mean, std, flat):
    """No column within a factor 2 of the flat threshold, on either side: two correct implementations of the
    definition then classify every column alike."""
    thr = 8 * np.longdouble(unit_roundoff(x.dtype)) * np.abs(mean)
    return bool(np.all(np.where(flat, 2 * std <= thr, std >= 2 * thr)))
