"""Direct tests of the flat-buffer kernels of csrc/flat_ops.hip through the C ABI: bsig_colsum (the slab
clamp of the 8 rows in flight, the two-stage path and its fallback), bsig_adam_flat (the float4 body, the
scalar tail, the grid stride of both loops) and bsig_normalize_rows (the grid wrap, both block sizes),
against fp64 with bounds derived next to the assertions, behind sentinel guards around every output.
u = 2^-24."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U24 = 2.0 ** -24
SENTINEL = 0x7FA5A5A5          # a NaN no kernel produces
GUARD = 64                     # floats of sentinel around an output
SECOND_ORDER = 1 + 2.0 ** -20  # the products of two rounding errors the first-order bounds leave out


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)


def untouched(t):
    return bool((t == SENTINEL).all())


def pitched(values, ld):
    """[rows, cols] values in a [max(rows, 1), ld] storage, the pitch beyond cols NaN"""
    rows, cols = values.shape
    store = torch.full((max(rows, 1), ld), float('nan'), device=DEV)
    store[:rows, :cols] = values
    return store


# --------------------------------------------------------------------- colsum
def _colsum(B, x, ld, rows, cols, ws_floats):
    """bsig_colsum into a guarded out; the workspace is ws_floats long with a sentinel tail.  Returns
    (out on the device, the workspace was left untouched)."""
    L, lib = B._lib, B._lib.load()
    buf = sentinel(GUARD + cols + GUARD)
    ws = sentinel(ws_floats + GUARD)
    out_ptr = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    L.check(lib.bsig_colsum(L.ptr(x), ld, rows, cols, out_ptr, L.ptr(ws), 4 * ws_floats, L.stream()))
    assert untouched(buf[:GUARD]) and untouched(buf[GUARD + cols:]), 'colsum wrote outside out[0:%d]' % cols
    assert untouched(ws[ws_floats:]), 'colsum wrote behind its workspace'
    return buf[GUARD:GUARD + cols].view(torch.float32).clone(), untouched(ws)


@pytest.mark.parametrize('rows', [0, 1, 31, 33, 1024, 1025, 40000])
def test_colsum(B, rows):
    """rows = 0: no slab at all; 1, 31, 33: the clamp inside a thread's 8 rows in flight; 1024: the last
    single-slab size; 1025: the first two-stage size (3 slabs); 40000: the cap of 64 slabs.  A workspace one
    float too small for the slabs falls back to one slab and stays untouched.  Integers in [-8, 8] sum
    exactly (40000 * 8 < 2^24); rows = 0 gives zeros.  Random inputs: a sum of `rows` terms in any order is
    within rows * 2^-24 * sum|x| of the exact one, per column."""
    gen = torch.Generator(device=DEV).manual_seed(100 + rows)
    slabs = 1 if rows <= 1024 else min(-(-rows // 512), 64)
    for cols in (1, 63, 64, 65, 260):
        for ld in (cols, cols + 3):
            ints = torch.randint(-8, 9, (rows, cols), device=DEV, generator=gen).float()
            reals = torch.randn(rows, cols, device=DEV, generator=gen)
            for ws_floats in ([slabs * cols, slabs * cols - 1] if slabs > 1 else [0]):
                staged = slabs > 1 and ws_floats == slabs * cols
                got, ws_clean = _colsum(B, pitched(ints, ld), ld, rows, cols, ws_floats)
                assert ws_clean == (not staged), (cols, ld, ws_floats)
                assert torch.equal(got, ints.double().sum(0).float()), (cols, ld, ws_floats)
                if rows == 0:
                    assert torch.equal(got, torch.zeros(cols, device=DEV))
                got, _ = _colsum(B, pitched(reals, ld), ld, rows, cols, ws_floats)
                ref = reals.double().sum(0)
                bound = rows * U24 * reals.double().abs().sum(0)
                assert ((got.double() - ref).abs() <= bound).all(), (cols, ld, ws_floats)
                if rows >= 33:
                    assert not torch.equal(got, torch.zeros_like(got))


# ----------------------------------------------------------------------- Adam
LR, BETA1, BETA2, EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))     # as the C floats arrive


def _adam_step(B, bufs, n, t):
    L, lib = B._lib, B._lib.load()
    L.check(lib.bsig_adam_flat(L.ptr(bufs['p']), L.ptr(bufs['g']), L.ptr(bufs['m']), L.ptr(bufs['v']), n,
                               LR, BETA1, BETA2, EPS, t, L.stream()))


def _adam_reference(p, g, m, v, t):
    """torch's single-tensor Adam as csrc/flat_ops.hip states it, in fp64 from the fp32 inputs, and the
    rounding-error bound of each output.  The two scalars are resolved on the host in double and rounded to
    fp32 once (adam_launch): the reference takes the same two fp32 numbers.
        m' = m + (g - m) (1 - b1)          two roundings: the difference, the fused multiply-add
        v' = v b2 + (1 - b2) g g           three: (1 - b2) g, and either v b2 or the product with g, then the
                                           fused multiply-add of the other
        p' = p - ss m' / (sqrt(v') ib + eps)   sqrt, product, sum, quotient, product, difference -- on the
                                           kernel's own m' and v', whose errors go through the formula
    (1 - b1 and 1 - b2 are exact in fp32: Sterbenz.)"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    ss = float(np.float32(LR / (1.0 - BETA1 ** t)))
    ib = float(np.float32(1.0 / np.sqrt(1.0 - BETA2 ** t)))
    omb1, omb2 = float(np.float32(1.0) - np.float32(BETA1)), float(np.float32(1.0) - np.float32(BETA2))
    d = g - m
    m1 = m + d * omb1
    e_m = U24 * (d.abs() * omb1 + m1.abs())
    gg = omb2 * g * g
    v1 = v * BETA2 + gg
    e_v = U24 * (gg + torch.maximum(v * BETA2, gg) + v1)
    s = torch.sqrt(v1)
    e_s = torch.where(v1 > 0, e_v / (2 * s).clamp_min(1e-300), torch.zeros_like(s)) + U24 * s
    prod = s * ib
    e_prod = e_s * ib + U24 * prod
    den = prod + EPS
    e_den = e_prod + U24 * den
    q = m1 / den
    e_q = e_m / den + q.abs() * e_den / den + U24 * q.abs()
    r = ss * q
    e_r = ss * e_q + U24 * r.abs()
    p1 = p - r
    e_p = e_r + U24 * p1.abs()
    return (p1, e_p * SECOND_ORDER), (m1, e_m * SECOND_ORDER), (v1, e_v * SECOND_ORDER)


def _adam_buffers(n, gen, zero):
    """p, g, m, v of n floats, 16-byte aligned, each with a sentinel-filled tail"""
    bufs = {}
    for name in ('p', 'g', 'm', 'v'):
        t = sentinel(n + GUARD).view(torch.float32)
        if zero and name != 'p':
            t[:n] = 0.0
        elif name == 'v':
            t[:n] = torch.rand(n, device=DEV, generator=gen) * 0.01
        else:
            t[:n] = torch.randn(n, device=DEV, generator=gen) * (0.1 if name == 'm' else 1.0)
        bufs[name] = t
    return bufs


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4 * 256 * 2048 + 7])
def test_adam_flat(B, n):
    """n = 1, 3: the scalar tail alone; 4: one float4; 5, 1023: both; 4 * 256 * 2048 + 7: more quads than the
    2048 x 256 threads of the grid (the float4 loop strides once) and a tail.  Steps 1, 2 and 1000; two
    consecutive steps on the same buffers; all-zero gradients on a zero state (0 / eps: the parameters do not
    move, bit for bit).  Elements at and beyond n are untouched."""
    gen = torch.Generator(device=DEV).manual_seed(7 + n)
    for t in (1, 2, 1000):
        bufs = _adam_buffers(n, gen, zero=False)
        for step in (t, t + 1):                      # the second step starts from the first one's fp32 outputs
            before = {name: bufs[name][:n].clone() for name in bufs}
            _adam_step(B, bufs, n, step)
            wants = _adam_reference(before['p'], before['g'], before['m'], before['v'], step)
            for name, (want, bound) in zip(('p', 'm', 'v'), wants):
                err = (bufs[name][:n].double() - want).abs()
                assert (err <= bound).all(), (n, step, name, float((err / bound.clamp_min(1e-300)).max()))
                assert not torch.equal(bufs[name][:n], before[name])
            assert torch.equal(bufs['g'][:n], before['g'])
            for name in bufs:
                assert untouched(bufs[name][n:].view(torch.int32)), (n, step, name)
        zeros = _adam_buffers(n, gen, zero=True)
        p0 = zeros['p'][:n].clone()
        _adam_step(B, zeros, n, t)
        assert torch.equal(zeros['p'][:n].view(torch.int32), p0.view(torch.int32))
        assert not zeros['m'][:n].any() and not zeros['v'][:n].any()
        for name in zeros:
            assert untouched(zeros[name][n:].view(torch.int32)), (n, t, name)


# ------------------------------------------------------------- normalize_rows
@pytest.mark.parametrize('rows', [1, 4097])
def test_normalize_rows(B, rows):
    """(theta - lows) / (highs - lows): two differences of fp32 inputs and a correctly rounded quotient, each
    within 2^-24 of its value: 3 u and the second-order terms, 4 * 2^-24 |out|.  4097 rows wrap the grid of
    4096 workgroups; 191 and 192 columns are either side of the block-size switch.  Padded pitches on both
    sides: the padding of out and the rows around it are untouched."""
    L, lib = B._lib, B._lib.load()
    gen = torch.Generator(device=DEV).manual_seed(3 + rows)
    for cols in (1, 3, 191, 192, 300):
        ld_in, ld_out = cols + 2, cols + 5
        lows = torch.randn(cols, device=DEV, generator=gen)
        highs = lows + 0.5 + torch.rand(cols, device=DEV, generator=gen)
        theta = lows + torch.rand(rows, cols, device=DEV, generator=gen) * (highs - lows)
        src = pitched(theta, ld_in)
        buf = sentinel((rows + 2) * ld_out)
        out_ptr = C.c_void_p(buf.data_ptr() + 4 * ld_out)
        L.check(lib.bsig_normalize_rows(L.ptr(src), ld_in, L.ptr(lows), L.ptr(highs), out_ptr, ld_out, rows, cols,
                                        L.stream()))
        body = buf.view(rows + 2, ld_out)
        got = body[1:rows + 1, :cols].view(torch.float32).clone()
        body[1:rows + 1, :cols] = SENTINEL
        assert untouched(buf), 'normalize_rows wrote outside out[0:%d, 0:%d]' % (rows, cols)
        want = (theta.double() - lows.double()) / (highs.double() - lows.double())
        err = (got.double() - want).abs()
        assert (err <= 4 * U24 * want.abs()).all(), (cols, float((err / (4 * U24 * want.abs()).clamp_min(1e-300)).max()))
        assert got.abs().max() > 0
