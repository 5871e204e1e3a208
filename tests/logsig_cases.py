"""What the log-signature tests compare with (include/bsig_logsignature.h), none of it the library's way:

  * the Lyndon words by their definition -- every word filtered by the rotation test, no Duval --, and
    Witt's formula for their number;
  * log S by the tensor-log SERIES, sum_n (-1)^(n+1)/n (S - 1)^(x)n in the truncated tensor algebra, in
    whatever numbers the signature comes in: exact ``Fraction``s, ``np.longdouble`` or ``np.float64``.  This is
    deliberately not the per-word sum over cuts that the kernel evaluates;
  * signatures by a restated Chen recursion in those numbers (``oracle.signature.signature`` serves fp64);
  * the term-wise magnitude A_w = sum over the cuts of w of (1/n) prod Sabs_ui, where Sabs is the signature of
    the path whose increments are the absolute values of this path's: what the error bounds scale with.

A signature is a 2-D array [rows, d + d^2 + ... + d^depth] (levels concatenated, C order); exact ones are
object arrays of Fractions.  No GPU, no library call."""
import itertools
from fractions import Fraction

import numpy as np


def lyndon_words(d, depth):
    """Words over 0 < 1 < ... < d-1 strictly smaller than all their proper rotations; by length, then
    lexicographically (itertools.product is lexicographic)."""
    words = []
    for k in range(1, depth + 1):
        for w in itertools.product(range(d), repeat=k):
            if all(w < w[r:] + w[:r] for r in range(1, k)):
                words.append(w)
    return words


def _moebius(n):
    res, p = 1, 2
    while p * p <= n:
        if n % p == 0:
            n //= p
            if n % p == 0:
                return 0
            res = -res
        p += 1
    return -res if n > 1 else res


def witt(d, depth):
    """sum_{k=1..depth} (1/k) sum_{e | k} mu(e) d^(k/e)"""
    total = 0
    for k in range(1, depth + 1):
        s = sum(_moebius(e) * d ** (k // e) for e in range(1, k + 1) if k % e == 0)
        assert s % k == 0
        total += s // k
    return total


def level_start(d, k):
    """Where level k starts in a signature row."""
    return sum(d ** j for j in range(1, k))


def word_offset(word, d):
    at = 0
    for letter in word:
        at = at * d + letter
    return level_start(d, len(word)) + at


def _one(sig):
    return Fraction(1) if sig.dtype == object else sig.dtype.type(1)


def _levels(sig, d, depth):
    """[rows, width] -> [level 0 (ones), level 1, ..., level depth], each [rows, d^k]"""
    n = sig.shape[0]
    unit = np.empty((n, 1), sig.dtype)
    unit[:] = _one(sig)
    return [unit] + [sig[:, level_start(d, k):level_start(d, k + 1)] for k in range(1, depth + 1)]


def _outer(a, b):
    return (a[:, :, None] * b[:, None, :]).reshape(a.shape[0], -1)


def chen(incs, depth):
    """Chen's identity, S <- S (x) exp(inc) per segment with exp(inc)_k = inc^(x)k / k!: ``incs`` [rows, L-1, d]
    (longdouble, float64 or an object array of Fractions) -> the signature in the same numbers."""
    n, _, d = incs.shape
    one = _one(incs)
    unit = np.empty((n, 1), incs.dtype)
    unit[:] = one
    zeros = lambda k: unit[:, :1].repeat(d ** k, axis=1) * (one - one)
    levels = [unit] + [zeros(k) for k in range(1, depth + 1)]
    for step in range(incs.shape[1]):
        expo = [unit]
        for k in range(1, depth + 1):
            expo.append(_outer(expo[-1], incs[:, step]) * (one / k))
        levels = [unit] + [sum(_outer(levels[j], expo[k - j]) for j in range(1, k + 1)) + expo[k]
                           for k in range(1, depth + 1)]
    return np.concatenate(levels[1:], axis=1)


def increments(paths, exact=False):
    """``paths`` [rows, L, d] (a double tensor or array) -> (incs, |incs|) in longdouble, or as Fractions."""
    x = np.asarray(paths, dtype=np.float64)
    if exact:
        frac = np.empty(x.shape, object)
        for at, v in np.ndenumerate(x):
            frac[at] = Fraction(float(v))
        x = frac
    else:
        x = x.astype(np.longdouble)
    incs = x[:, 1:] - x[:, :-1]
    return incs, abs(incs)


def log_series(sig, d, depth):
    """log S = sum_{n=1..depth} (-1)^(n+1)/n X^(x)n with X = S - 1 (no level 0), truncated at ``depth``: the
    full log tensor, [rows, width], in the numbers of ``sig``."""
    one = _one(sig)
    x = _levels(sig, d, depth)
    zero = x[0] * (one - one)
    x[0] = zero
    power = list(x)                    # X^(x)n, whose lowest level is n
    acc = list(x)
    for n in range(2, depth + 1):
        nxt = [zero]
        for k in range(1, depth + 1):
            terms = [_outer(power[i], x[k - i]) for i in range(n - 1, k)]       # x has no level 0
            nxt.append(sum(terms) if terms else power[k] * (one - one))
        power = nxt
        coef = (one / n) if n % 2 else -(one / n)
        acc = [a + p * coef for a, p in zip(acc, power)]
    return np.concatenate(acc[1:], axis=1)


def at_words(full, words, d):
    return full[:, [word_offset(w, d) for w in words]]


def logsignature(sig, d, depth, words=None):
    """The log-signature rows at the Lyndon words, by the series."""
    return at_words(log_series(sig, d, depth), lyndon_words(d, depth) if words is None else words, d)


def cuts(word):
    """Every way to cut ``word`` into consecutive non-empty pieces: lists of pieces."""
    k = len(word)
    for mask in range(1 << (k - 1)):
        pieces, start = [], 0
        for j in range(k):
            if j == k - 1 or (mask >> j) & 1:
                pieces.append(word[start:j + 1])
                start = j + 1
        yield pieces


def magnitude(sabs, words, d):
    """A_w = sum over the cuts of w of (1/n) prod Sabs_ui, per row: [rows, len(words)]."""
    one = _one(sabs)
    out = np.empty((sabs.shape[0], len(words)), sabs.dtype)
    for col, w in enumerate(words):
        acc = sabs[:, 0] * (one - one)
        for pieces in cuts(w):
            prod = sabs[:, word_offset(pieces[0], d)]
            for u in pieces[1:]:
                prod = prod * sabs[:, word_offset(u, d)]
            acc = acc + prod * (one / len(pieces))
        out[:, col] = acc
    return out
