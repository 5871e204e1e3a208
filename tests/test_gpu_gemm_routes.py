"""Every route of bsig_gemm_f32 (csrc/gemm_f32.hip: gemm_mfma_kernel, gemm_lean_kernel, the two whole-width
kernels, gemm_f64acc_kernel, the three reduce kernels) on the rows of tests/gemm_cases.py: each call first
asserts the route bsig_debug_gemm_path reports, runs behind guards -- c sits in a sentinel-filled buffer
with a guard row in front, two behind and the pitch beyond the columns; the workspace has a sentinel tail
-- and is compared with the fp64 product: bit for bit where the arithmetic is exact, inside a derived bound
elsewhere.  u = 2^-24."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U24, U23 = 2.0 ** -24, 2.0 ** -23
SENTINEL = 0x7FA5A5A5          # a NaN no kernel produces
WS_TAIL = 4096                 # bytes behind the workspace the call was told about
LDC_MODES = ('tight', 'plus1', 'pad4')
EPI_NONE, EPI_BIAS, EPI_BIAS_ACT, EPI_COS_SIN, EPI_COS_OFF, EPI_MUL_DACT = range(6)
ACT_TANH, ACT_RELU, ACT_LEAKY_RELU, ACT_SIGMOID = range(4)


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    return pkg


@contextlib.contextmanager
def environment(env):
    old = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for key, val in old.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val


def path(B, m, n, k, akm, bkm, gathered, epi, ws_bytes):
    out = (C.c_int32 * 8)()
    assert B._lib.load().bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, ws_bytes, 0, out) == 0
    return list(out)


def ws_bytes_of(B, c):
    return int(B._lib.load().bsig_gemm_workspace_bytes(c.m, c.n, c.k)) if c.ws is None else c.ws


def assert_route(B, c, epi, ws_bytes):
    """the row's route, as tests/test_gemm_cases_host.py asserts it (the environment is already set)"""
    got = path(B, c.m, c.n, c.k, c.akm, c.bkm, int(bool(c.gather)), epi, ws_bytes)
    if c.kernel_from_debug:
        assert got[0] == c.kernel, (G.case_id(c), got)
    assert got[1:4] == [c.tile_m, c.tile_n, c.splits], (G.case_id(c), got)


def ldc_of(mode, cols):
    return {'tight': cols, 'plus1': cols + 1, 'pad4': G.round_up(cols, 4) + 4}[mode]


def guarded_gemm(B, a, lda, akm, a_rows, b, ldb, bkm, b_rows, m, n, k, ws_bytes, epi=EPI_NONE, act=0, bias=None,
                 aux=None, alpha=1.0, ldc_mode='tight', offset=False, ws_untouched=False):
    """bsig_gemm_f32 into c[0:m, 0:cols] of a sentinel-filled buffer: one guard row in front, two behind,
    the pitch beyond cols (and one float in front when `offset`).  Afterwards, bit for bit: everything
    outside c[0:m, 0:cols] is still the sentinel, and so is the workspace behind ws_bytes (all of it with
    `ws_untouched`: an unsplit product has no business there).  Returns c[0:m, 0:cols] on the host."""
    L, lib = B._lib, B._lib.load()
    cols = 2 * n if epi == EPI_COS_SIN else n
    ldc = ldc_of(ldc_mode, cols)
    lead = ldc + (1 if offset else 0)
    buf = torch.full(((m + 3) * ldc + 4,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((ws_bytes // 4 + WS_TAIL // 4,), SENTINEL, dtype=torch.int32, device=DEV)
    c_ptr = C.c_void_p(buf.data_ptr() + 4 * lead)
    L.check(lib.bsig_gemm_f32(L.ptr(a), lda, akm, L.ptr(a_rows), L.ptr(b), ldb, bkm, L.ptr(b_rows), c_ptr, ldc,
                              m, n, k, epi, act, L.ptr(bias), L.ptr(aux), aux.stride(0) if aux is not None else 0,
                              alpha, L.ptr(ws), ws_bytes, L.stream()))
    host = buf.cpu()
    body = host[lead:lead + (m + 2) * ldc].view(m + 2, ldc)
    got = body[:m, :cols].clone()
    body[:m, :cols] = SENTINEL
    stray = (host != SENTINEL).nonzero().flatten()
    assert stray.numel() == 0, 'written outside c[0:%d, 0:%d] (ldc %d): flat offsets %s' % (
        m, cols, ldc, (stray[:8] - lead).tolist())
    tail = ws if ws_untouched else ws[ws_bytes // 4:]
    assert bool((tail == SENTINEL).all()), 'workspace written %s' % ('by an unsplit product' if ws_untouched
                                                                      else 'behind its end')
    return got.view(torch.float32)


def make_operand(logical, kmajor, gather, ld, gen, repeat=True):
    """Device storage of the logical [rows, k] operand (see tests/gemm_cases.py): k-contiguous [rows, k] or
    k-major [k, rows] at a pitch of `ld` floats, the pitch beyond the operand NaN; gathered: through an index
    vector with out-of-order entries into a larger shuffled storage, and (repeat) rows 0 and g - 1 of the
    gathered dimension the same source row -- `logical` is updated in place to what the kernel then sees."""
    mat = logical.T.contiguous() if kmajor else logical.contiguous()       # [gathered dim, other]
    g, w = mat.shape
    assert ld >= w
    rows = None
    store = torch.full((g + (3 if gather else 0), ld), float('nan'), dtype=torch.float32)
    if gather:
        perm = torch.randperm(g + 3, generator=gen)
        rows = perm[:g].clone()
        store[:, :w] = torch.randn(g + 3, w, generator=gen)
        if repeat and g > 2:
            mat[g - 1] = mat[0]
            rows[g - 1] = rows[0]
            logical.copy_(mat.T if kmajor else mat)
        store[rows, :w] = mat
        rows = rows.to(torch.int32).to(DEV)
    else:
        store[:, :w] = mat
    return store.to(DEV), rows


class Operands:
    """the two operands of a row on the device, their logical values on the host"""

    def __init__(self, c, a_t, b_t, gen, repeat_a=True, repeat_b=True):
        self.lda, self.ldb = G.pitches(c)
        self.a, self.a_rows = make_operand(a_t, c.akm, 'a' in c.gather, self.lda, gen, repeat_a)
        self.b, self.b_rows = make_operand(b_t, c.bkm, 'b' in c.gather, self.ldb, gen, repeat_b)
        self.a_t, self.b_t = a_t, b_t


def operand_key(c):
    return (c.m, c.n, c.k, c.akm, c.bkm, c.gather, c.lda, c.ldb)


def seed_of(c, salt):
    return 1000003 * salt + 7919 * c.m + 104729 * c.n + 31 * c.k + 8 * c.akm + 4 * c.bkm + len(c.gather)


def run_case(B, c, ops, ldc_mode='tight', offset=False, epi=None, **kw):
    epi = c.epi if epi is None else epi
    ws_bytes = ws_bytes_of(B, c)
    with environment(c.env):
        assert_route(B, c, epi, ws_bytes)
        generic_unsplit = c.kernel in (G.MFMA, G.LEAN, G.F64ACC) and c.splits == 1
        return guarded_gemm(B, ops.a, ops.lda, c.akm, ops.a_rows, ops.b, ops.ldb, c.bkm, ops.b_rows, c.m, c.n, c.k,
                            ws_bytes, epi=epi, ldc_mode=ldc_mode, offset=offset, ws_untouched=generic_unsplit, **kw)


def zero_bias(c):
    return torch.zeros(c.n, device=DEV) if c.epi == EPI_BIAS else None


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize('group', G.GROUPS)
def test_small_integers_are_exact(B, group):
    """Integers in [-8, 8]: every product is at most 64 and every partial sum at most 2080 * 64 < 2^24, so
    every route, every summation order and every K split returns the integer product.  Every row runs at
    ldc = cols, cols + 1 (the scalar epilogue) and round_up(cols, 4) + 4 (the 16-byte one beside padding),
    a subset with c one float off; and with the exact epilogues: an integer bias, bias + ReLU and the ReLU
    derivative of an aux in {0, 1, 2} (the whole-width forward rows carry the two epilogues that route takes)."""
    cache = {}
    for i, c in enumerate(G.group(group)):
        key = operand_key(c)
        if key not in cache:
            gen = torch.Generator().manual_seed(seed_of(c, 1))
            a_t = torch.randint(-8, 9, (c.m, c.k), generator=gen).float()
            b_t = torch.randint(-8, 9, (c.n, c.k), generator=gen).float()
            ops = Operands(c, a_t, b_t, gen)
            bias_t = torch.randint(-8, 9, (c.n,), generator=gen).float()
            aux_t = torch.randint(0, 3, (c.m, G.round_up(c.n, 4)), generator=gen).float()
            cache[key] = (ops, (a_t.double() @ b_t.double().T).float(), bias_t, aux_t)
        ops, want, bias_t, aux_t = cache[key]
        bias, aux = bias_t.to(DEV), aux_t.to(DEV)[:, :c.n]
        if c.epi == EPI_BIAS:
            kw, expect = dict(bias=bias), want + bias_t
        else:
            kw, expect = {}, want
        for mode in LDC_MODES:
            got = run_case(B, c, ops, mode, **kw)
            assert torch.equal(got, expect), (G.case_id(c), mode)
        if c.c_offset:
            got = run_case(B, c, ops, 'tight', offset=True, **kw)
            assert torch.equal(got, expect), (G.case_id(c), 'offset')
        if group.startswith('wide-forward'):
            continue
        mode = LDC_MODES[i % 3]
        got = run_case(B, c, ops, mode, epi=EPI_BIAS, bias=bias)
        assert torch.equal(got, want + bias_t), (G.case_id(c), 'bias')
        got = run_case(B, c, ops, LDC_MODES[(i + 1) % 3], epi=EPI_BIAS_ACT, act=ACT_RELU, bias=bias)
        assert torch.equal(got, torch.relu(want + bias_t)), (G.case_id(c), 'bias relu')
        got = run_case(B, c, ops, LDC_MODES[(i + 2) % 3], epi=EPI_MUL_DACT, act=ACT_RELU, aux=aux)
        assert torch.equal(got, want * (aux_t[:, :c.n] > 0).float()), (G.case_id(c), 'relu derivative')


def full_mantissa(shape, gen):
    """fp32 values with 24 random mantissa bits, a random sign and an exponent in [-100, 100]"""
    mant = torch.randint(1 << 23, 1 << 24, shape, generator=gen).double()
    expo = torch.randint(-100, 101, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    x = (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo - 23)).float()
    assert torch.isfinite(x).all() and (x != 0).all()
    return x


def selection(rows, k, gen):
    sel = torch.randint(0, k, (rows,), generator=gen)
    mat = torch.zeros(rows, k)
    mat[torch.arange(rows), sel] = 1.0
    return mat, sel


@pytest.mark.parametrize('group', G.GROUPS)
def test_selection_returns_every_bit(B, group):
    """One operand with full 24-bit mantissas, random signs and exponents in [-100, 100] against a 0/1
    selection matrix, both ways round: c is the selected entries bit for bit -- every other term of a sum is
    a zero.  A transposed fragment, a wrong gather index, a K tail that is not zeroed (the pitch behind it is
    NaN) all fail here with no tolerance.  (The selection operand is gathered without the repeated row: a
    repeated contraction row would select two entries.)  The ldc form rotates through the rows."""
    cache = {}
    for i, c in enumerate(G.group(group)):
        key = operand_key(c)
        if key not in cache:
            gen = torch.Generator().manual_seed(seed_of(c, 2))
            a_t = full_mantissa((c.m, c.k), gen)
            b_t, sel = selection(c.n, c.k, gen)
            fwd = Operands(c, a_t, b_t, gen, repeat_b=False)
            want_fwd = a_t[:, sel].contiguous()
            b2_t = full_mantissa((c.n, c.k), gen)
            a2_t, sel_m = selection(c.m, c.k, gen)
            rev = Operands(c, a2_t, b2_t, gen, repeat_a=False)
            want_rev = b2_t[:, sel_m].T.contiguous()
            cache[key] = (fwd, want_fwd, rev, want_rev)
        fwd, want_fwd, rev, want_rev = cache[key]
        mode = LDC_MODES[i % 3]
        offset = c.c_offset and i % 2 == 0
        got = run_case(B, c, fwd, mode, offset=offset, bias=zero_bias(c))
        assert torch.equal(got.view(torch.int32), want_fwd.view(torch.int32)), (G.case_id(c), mode, 'A carries')
        got = run_case(B, c, rev, mode, offset=offset, bias=zero_bias(c))
        assert torch.equal(got.view(torch.int32), want_rev.view(torch.int32)), (G.case_id(c), mode, 'B carries')


# ---------------------------------------------------------------------- error
@pytest.mark.parametrize('dist', ['normal', 'positive'])
@pytest.mark.parametrize('group', G.GROUPS)
def test_error_against_fp64(B, group, dist):
    """|C - C64| <= (k + 8) 2^-23 (|A| |B|): a sum of k exact-product fmas in any order is within gamma_k of
    the magnitude sum; the at most 27 slab additions and the final rounding are inside the + 8 once the unit
    is 2^-23 instead of 2^-24 -- the rounding inside the 16x16x4 MFMA's four-term sum is not documented
    (tests/test_gpu_matmul.py takes the same stance).  gemm_f64acc_kernel: 2^-24 |C64| + k 2^-53 (|A| |B|),
    one rounding of an fp64 sum.  The same call twice is bitwise the same; the lean kernel is bitwise
    gemm_mfma_kernel on the same plan; a whole-width route and the generic route on the same inputs both
    satisfy the bound (another summation order: not bitwise equal)."""
    cache, worst = {}, {}
    for i, c in enumerate(G.group(group)):
        key = operand_key(c)
        if key not in cache:
            gen = torch.Generator().manual_seed(seed_of(c, 3))
            draw = (lambda *s: torch.randn(*s, generator=gen)) if dist == 'normal' else \
                (lambda *s: torch.rand(*s, generator=gen) + 0.01)
            a_t, b_t = draw(c.m, c.k), draw(c.n, c.k)
            ops = Operands(c, a_t, b_t, gen)
            ref = a_t.double() @ b_t.double().T
            mag = a_t.double().abs() @ b_t.double().abs().T
            cache[key] = (ops, ref, mag)
        ops, ref, mag = cache[key]
        if c.kernel == G.F64ACC:
            bound = U24 * ref.abs() + c.k * 2.0 ** -53 * mag
        else:
            bound = (c.k + 8) * U23 * mag
        mode = LDC_MODES[i % 3]
        got = run_case(B, c, ops, mode, bias=zero_bias(c))
        err = (got.double() - ref).abs()
        ratio = float((err / bound).max())
        worst[G.KERNEL_NAMES[c.kernel]] = max(worst.get(G.KERNEL_NAMES[c.kernel], 0.0), ratio)
        assert (err <= bound).all(), (G.case_id(c), ratio)
        again = run_case(B, c, ops, mode, bias=zero_bias(c))
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), G.case_id(c)
        if c.kernel == G.LEAN:
            old = c._replace(env=dict(c.env, BSIG_GEMM_LEAN='0'), kernel=G.MFMA)
            other = run_case(B, old, ops, mode, bias=zero_bias(c))
            assert torch.equal(got.view(torch.int32), other.view(torch.int32)), G.case_id(c)
        if c.kernel in (G.WIDE_FORWARD, G.WIDE_GRADIENT):
            with environment({'BSIG_GEMM_WIDE': '0'}):
                ws_bytes = ws_bytes_of(B, c)
                route = path(B, c.m, c.n, c.k, c.akm, c.bkm, int(bool(c.gather)), c.epi, ws_bytes)
                assert route[0] in (G.MFMA, G.LEAN), route
                other = guarded_gemm(B, ops.a, ops.lda, c.akm, ops.a_rows, ops.b, ops.ldb, c.bkm, ops.b_rows,
                                     c.m, c.n, c.k, ws_bytes, epi=c.epi, bias=zero_bias(c), ldc_mode=mode)
            assert ((other.double() - ref).abs() <= bound).all(), G.case_id(c)
    for name, ratio in sorted(worst.items()):
        print('%s %s: largest error / bound on %s = %.4f' % (group, dist, name, ratio))


def _route_rows():
    """one row per kernel id"""
    rows = {}
    for c in G.CASES:
        if c.kernel_from_debug and c.k >= 130 and (c.m > 37 or c.kernel == G.F64ACC) and c.n > 5 and c.epi == EPI_NONE:
            rows.setdefault(c.kernel, c)
    assert sorted(rows) == [G.MFMA, G.LEAN, G.WIDE_FORWARD, G.WIDE_GRADIENT, G.F64ACC]
    return [rows[key] for key in sorted(rows)]


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('c', _route_rows(), ids=lambda c: G.KERNEL_NAMES[c.kernel])
def test_nonfinite_operand_element(B, c, bad):
    """One inf / NaN in A and one in B on each of the five routes: exactly the affected row and column of c
    are non-finite."""
    if c.kernel == G.F64ACC:
        c = c._replace(m=70, tile_m=0)        # (the table's 33 rows do not reach row 37)
    gen = torch.Generator().manual_seed(11)
    a_t, b_t = torch.randn(c.m, c.k, generator=gen), torch.randn(c.n, c.k, generator=gen)
    a_t[37, 100] = bad
    b_t[5, c.k // 2] = bad
    ops = Operands(c, a_t, b_t, gen)
    assert not torch.isfinite(ops.a_t[37]).all() and not torch.isfinite(ops.b_t[5]).all()
    got = run_case(B, c, ops, 'pad4')
    hit = torch.zeros(c.m, c.n, dtype=torch.bool)
    hit[37, :] = True
    hit[:, 5] = True
    assert not torch.isfinite(got[hit]).any() and torch.isfinite(got[~hit]).all()


# ------------------------------------------------------------------ epilogues
EPILOGUES = ['bias', 'bias_tanh', 'bias_relu', 'bias_leaky', 'bias_sigmoid', 'cos_sin', 'cos_off',
             'dact_tanh', 'dact_relu', 'dact_leaky', 'dact_sigmoid']
# interior tiles only / ragged in M, N and K (n % 4 = 2: the scalar form of every epilogue, COS_SIN at
# ldc = 144 > 2 n among them).  k-contiguous operands, and both k-major: (130, 70, 257) k-major sits at
# pitches of 144 and 72 floats, where the lean kernel runs it (the debug entry takes B as dense [k, 70]
# and cannot name the kernel there).
EPI_SHAPES = [(128, 128, 64, 0, 0, 0, 0, True), (128, 128, 64, 1, 1, 0, 0, True),
              (130, 70, 257, 0, 0, 0, 0, True), (130, 70, 257, 1, 1, 144, 72, False)]


def _epilogue_reference(epi, pre, bias_t, aux_t, alpha):
    """(call arguments, fp64 result, Lipschitz constant, argument of the function, exact) of one epilogue on
    the exact accumulator `pre`"""
    bd, h = bias_t.double(), aux_t.double()
    arg = pre + bd
    p32, b32, h32 = pre.float().numpy(), bias_t.numpy(), aux_t.numpy()
    v32 = p32 + b32                                  # fp32: what the kernel adds
    if epi == 'bias':
        return dict(epi=EPI_BIAS), arg, 1.0, arg, None
    if epi == 'bias_tanh':
        return dict(epi=EPI_BIAS_ACT, act=ACT_TANH), torch.tanh(arg), 1.0, arg, None
    if epi == 'bias_relu':
        return dict(epi=EPI_BIAS_ACT, act=ACT_RELU), torch.relu(arg), 1.0, arg, None
    if epi == 'bias_leaky':     # one correctly rounded fp32 product: the numpy float32 result exactly
        return dict(epi=EPI_BIAS_ACT, act=ACT_LEAKY_RELU), None, 0.0, arg, np.where(v32 > 0, v32, np.float32(0.01) * v32)
    if epi == 'bias_sigmoid':
        return dict(epi=EPI_BIAS_ACT, act=ACT_SIGMOID), torch.sigmoid(arg), 0.25, arg, None
    if epi == 'cos_sin':
        return dict(epi=EPI_COS_SIN), alpha * torch.cat([torch.cos(pre), torch.sin(pre)], 1), alpha, \
            torch.cat([pre, pre], 1), None
    if epi == 'cos_off':
        return dict(epi=EPI_COS_OFF), alpha * torch.cos(arg), alpha, arg, None
    if epi == 'dact_tanh':
        return dict(epi=EPI_MUL_DACT, act=ACT_TANH), pre * (1 - h * h), None, pre, None
    if epi == 'dact_sigmoid':
        return dict(epi=EPI_MUL_DACT, act=ACT_SIGMOID), pre * (h * (1 - h)), None, pre, None
    if epi == 'dact_relu':
        return dict(epi=EPI_MUL_DACT, act=ACT_RELU), None, 0.0, pre, p32 * (h32 > 0).astype(np.float32)
    assert epi == 'dact_leaky'
    return dict(epi=EPI_MUL_DACT, act=ACT_LEAKY_RELU), None, 0.0, pre, \
        p32 * np.where(h32 > 0, np.float32(1.0), np.float32(0.01))


@pytest.mark.parametrize('epi', EPILOGUES)
def test_fused_and_reduced_epilogues(B, epi):
    """Every epilogue where the kernel applies it itself (no workspace: one slice -- tile_epilogue_vec on
    interior tiles at a 16-byte pitch, tile_epilogue on edge tiles and at ldc = cols + 1) and where
    gemm_reduce_kernel applies it (>= 2 slices), on gemm_mfma_kernel and gemm_lean_kernel.  The operands are
    multiples of 1/8 of magnitude <= 1: the accumulator is exact and the bound is the epilogue's own fp32
    evaluation, the formula of tests/test_gpu_matmul.py::test_epilogues with g = 0:
        Lip 2^-24 |arg| + 4 * 2^-24 |want|.
    MUL_DACT with tanh / sigmoid: 3 * 2^-24 |want| (two roundings in 1 - h h or h (1 - h), with or without
    contraction, one in the product).  ReLU and leaky ReLU (one correctly rounded fp32 product) are compared
    with the numpy float32 result exactly."""
    alpha = 0.25
    for (m, n, k, akm, bkm, lda, ldb, from_debug) in EPI_SHAPES:
        gen = torch.Generator().manual_seed(29 + m + akm)
        a_t = torch.randint(-8, 9, (m, k), generator=gen).float() / 8
        b_t = torch.randint(-8, 9, (n, k), generator=gen).float() / 8
        bias_t = torch.randn(n, generator=gen)
        if epi == 'dact_sigmoid':
            aux_t = torch.randint(1, 8, (m, G.round_up(n, 4)), generator=gen).float() / 8
        elif epi == 'dact_relu':
            aux_t = torch.randint(0, 3, (m, G.round_up(n, 4)), generator=gen).float()
        else:
            aux_t = torch.randint(-7, 8, (m, G.round_up(n, 4)), generator=gen).float() / 8
        pre = a_t.double() @ b_t.double().T
        assert torch.equal(pre.float().double(), pre)            # the accumulator is exact
        kw, want, lip, arg, exact = _epilogue_reference(epi, pre, bias_t, aux_t[:, :n], alpha)
        if kw['epi'] in (EPI_BIAS, EPI_BIAS_ACT, EPI_COS_OFF):
            kw['bias'] = bias_t.to(DEV)
        if kw['epi'] == EPI_MUL_DACT:
            kw['aux'] = aux_t.to(DEV)[:, :n]
        if kw['epi'] in (EPI_COS_SIN, EPI_COS_OFF):
            kw['alpha'] = alpha
        if want is not None:
            bound = 3 * U24 * want.abs() if lip is None else lip * U24 * arg.abs() + 4 * U24 * want.abs() + 1e-30
        for lean in ('0', '1'):
            # (128, 128, 64): the planner takes one slice whatever the workspace (k / 128 = 0): two are forced
            for fused, env in ((True, {}), (False, {'BSIG_GEMM_SPLITS': '2'} if k == 64 else {})):
                tile = (128, 32) if m <= 128 else (64, 64)
                c = G._case('epilogue', m, n, k, akm, bkm, lda=lda, ldb=ldb, env=dict(env, BSIG_GEMM_LEAN=lean),
                            ws=0 if fused else None, tile=tile, splits=1 if fused else 2, kernel_from_debug=from_debug)
                ops = Operands(c, a_t, b_t, gen)
                for mode in LDC_MODES:
                    with environment(c.env):
                        slices = path(B, m, n, k, akm, bkm, 0, kw['epi'], ws_bytes_of(B, c))[3]
                        assert slices == 1 if fused else slices >= 2
                    got = run_case(B, c, ops, mode, **kw)
                    where = (epi, (m, n, k, akm, bkm), 'lean' + lean, 'fused' if fused else 'reduced', mode)
                    if exact is not None:
                        assert np.array_equal(got.numpy().view(np.int32), exact.astype(np.float32).view(np.int32)), where
                    else:
                        err = (got.double() - want).abs()
                        assert got.shape == want.shape and (err <= bound).all(), (where, float((err / bound).max()))
