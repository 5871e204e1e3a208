"""The definition of include/bsig_rff_bandwidth.h restated in numpy, and the value patterns of the selection
tests.  The squared distances are summed in long double (64 mantissa bits on x86, more elsewhere) and rounded
once, so the reference is within half an ulp of the exact sum; the kernel's chain of ``width`` fma is within
(width + 2) 2^-53 relative of it because every term is non-negative."""
import numpy as np

MAX_ROWS = 1024
SELECT_WORKSPACE_BYTES = 8448
U53 = np.longdouble(2.0) ** -53
assert np.finfo(np.longdouble).nmant >= 63, 'the reference needs a long double wider than a double'


def lower_median(v):
    """The element of 0-based rank (len - 1) // 2 of the ascending values; NaN if any is non-finite."""
    v = np.asarray(v, dtype=np.float64)
    if not np.isfinite(v).all():
        return np.float64('nan')
    return np.sort(v)[(v.size - 1) // 2]


def pair_d2(x, work=np.longdouble):
    """d2 of every pair i < j of the first MAX_ROWS rows, in long double (``work=np.float64``: in double, which
    is the kernel's own arithmetic where a row pair differs in ONE column -- one subtraction, one rounded square,
    zeros added)."""
    x = np.asarray(x)[:MAX_ROWS].astype(work)
    m = x.shape[0]
    out = []
    for i in range(m - 1):
        diff = x[i + 1:] - x[i]
        out.append((diff * diff).sum(axis=1))
    return np.concatenate(out)


def sigma2_ref(x, scale=1.0):
    """(scale * median distance)^2 in long double: what the square of the kernel's sigma is held against.
    None where the definition gives a special value (1.0 or NaN)."""
    with np.errstate(invalid='ignore', over='ignore'):
        d2 = pair_d2(x)
    if not np.isfinite(d2).all():
        return None
    med = np.sort(d2)[(d2.size - 1) // 2]
    return None if med == 0 else np.longdouble(scale) ** 2 * med


def sigma_ref(x, scale=1.0, work=np.longdouble):
    """sigma by the definition, in double: one sqrt, one multiplication."""
    with np.errstate(invalid='ignore', over='ignore'):
        d2 = pair_d2(x, work).astype(np.float64)
    if not np.isfinite(d2).all():
        return np.float64('nan')
    med = np.sort(d2)[(d2.size - 1) // 2]
    return np.float64(1.0) if med == 0 else np.float64(scale) * np.sqrt(med)


def within_bound(sigma, x, scale, width):
    """|sigma^2 - ref^2| <= (width + 4) 2^-53 ref^2"""
    ref2 = sigma2_ref(x, scale)
    got2 = np.longdouble(sigma) ** 2
    return ref2 is not None and abs(got2 - ref2) <= (width + 4) * U53 * ref2


SELECT_COUNTS = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 130816]
SELECT_PATTERNS = ['uniform', 'all_equal', 'two_low', 'two_high', 'half_tied', 'zeros_denormals', 'low_byte',
                   'exponent', 'every_digit']


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def select_values(pattern, count, seed=0):
    """``count`` non-negative finite doubles of the named pattern."""
    rng = np.random.RandomState(seed + 31 * count)
    if pattern == 'uniform':
        return rng.rand(count) * 1e3
    if pattern == 'all_equal':
        return np.full(count, 2.5)
    if pattern in ('two_low', 'two_high'):          # two distinct values, the majority below / above
        low = rng.rand(count) < (0.7 if pattern == 'two_low' else 0.3)
        return np.where(low, 1.25, 7.0)
    if pattern == 'half_tied':                       # half of the values are the median itself
        v = np.full(count, 3.0)
        rest = count - (count + 1) // 2
        v[:rest // 2] = rng.rand(rest // 2)
        v[rest // 2:rest] = 4.0 + rng.rand(rest - rest // 2)
        return rng.permutation(v)
    if pattern == 'zeros_denormals':
        v = _from_bits(rng.randint(0, 1 << 20, count).astype(np.uint64))     # denormals
        v[rng.rand(count) < 0.4] = 0.0
        return v
    if pattern == 'low_byte':                        # differ only in the lowest mantissa byte
        return _from_bits(np.float64(1.5).view(np.uint64) + rng.randint(0, 256, count).astype(np.uint64))
    if pattern == 'exponent':                        # differ only in the exponent
        return _from_bits(rng.randint(1, 2046, count).astype(np.uint64) << np.uint64(52))
    if pattern == 'every_digit':
        # each value shares a random number (0 .. 7) of top bytes with a base and has a random next byte: where
        # the count allows, every pass of an 8-bit radix select has to tell values apart; the exponent stays finite
        base = np.uint64(0x3FE5A4C3B2A19080)
        keep = rng.randint(0, 8, count)
        digit = rng.randint(0, 256, count).astype(np.uint64)
        noise = rng.randint(0, 1 << 62, count).astype(np.uint64)
        bits = np.empty(count, dtype=np.uint64)
        for i in range(count):
            shift = np.uint64(56 - 8 * keep[i])
            high = (base >> shift) >> np.uint64(8) << np.uint64(8) | digit[i]
            low_mask = (np.uint64(1) << shift) - np.uint64(1)
            bits[i] = (high << shift) | (noise[i] & low_mask)
        bits &= np.uint64(0x7FFFFFFFFFFFFFFF)
        bits[(bits >> np.uint64(52)) == np.uint64(0x7FF)] = base        # (never inf / NaN)
        return _from_bits(bits)
    raise KeyError(pattern)


def line_rows(n, width, dtype, column=0):
    """Rows on a line, x_i = 3^i in one column and zero elsewhere.  Every value and every difference is exact in
    double for n <= 33 (3^32 < 2^53) and in fp32 for n <= 15 (3^14 < 2^24); a pair's d2 is then ONE rounded
    square with zeros added, the same on any machine, and the differences lie far enough apart (relative gap
    >= 2 / 3^32 > 4 ulp) for all d2 to be distinct: a dropped or doubled pair moves the median elsewhere."""
    x = np.zeros((n, width), dtype=dtype)
    x[:, column] = np.asarray([3.0 ** i for i in range(n)], dtype=dtype)
    return x
