"""GPU checks of the split-bf16 matmul precision (include/bsig_matmul.h) through the C ABI and the public
Python switches: exactness where the arithmetic is exact, the error against the fp64 product (a derived
guard, and the fp32 kernel's own error as the yardstick), reproducibility, non-finite operands, every
epilogue, the RFF projection at the project's tolerance, and teacher-forced fits against the reference's
own outputs at the 1e-4 north star.

u = 2^-24.  The guard of the error tests: a chain of 6K sequential fp32 additions of exact products (unit
roundoff taken as 2^-23: the rounding of the MFMA's internal 16-term sum is not documented), 8 more for the
K slices, and 2^-23 for the dropped piece products (< 3 * 2.01 * 2^-24 per term):
    |C - C64| <= ((6K + 8) 2^-23 + 2^-23) (|A| |B|)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the last shape: 13 x 16 = 208 tiles of 128 x 128, the smallest class of products the planner gives the
# 128 x 128 instantiations (split_bf16_plan: at least 192 such tiles) -- ragged in m, k no multiple of 32
BIG = (1600, 2048, 300)
SHAPES = [(1, 1, 1), (33, 17, 50), (130, 70, 257), (64, 260, 1040), BIG]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
U23 = 2.0 ** -23


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@pytest.fixture(autouse=True)
def _guard(monkeypatch):
    import bayes_sim_ig_amd as pkg
    monkeypatch.delenv('BSIG_MATMUL_PRECISION', raising=False)
    old = pkg.MDNN.EPS_NOISE
    yield
    pkg.MDNN.EPS_NOISE = old
    pkg.MDNN.USE_GRAPH = True


def _path(B, m, n, k, akm, bkm, gathered, epi, ws_bytes, matmul=1):
    out = (C.c_int32 * 8)()
    assert B._lib.load().bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, ws_bytes, matmul, out) == 0
    return list(out)


def _gemm(B, a, b, m, n, k, a_km, b_km, matmul, epi=0, act=0, bias=None, aux=None, alpha=1.0,
          a_rows=None, b_rows=None, slabs=None):
    """bsig_gemm_f32_ex (matmul = None: bsig_gemm_f32).  ``slabs``: the workspace holds that many [m, n]
    slabs (default: what bsig_gemm_workspace_bytes asks for)."""
    L, lib = B._lib, B._lib.load()
    cols = 2 * n if epi == L.EPI_COS_SIN else n
    c = torch.full((m, cols), float('nan'), device=DEV)
    ws_bytes = int(lib.bsig_gemm_workspace_bytes(m, n, k)) if slabs is None else slabs * 4 * m * n
    ws = torch.empty(ws_bytes // 4 + 1, device=DEV)
    args = (L.ptr(a), a.stride(0), a_km, L.ptr(a_rows), L.ptr(b), b.stride(0), b_km, L.ptr(b_rows),
            L.ptr(c), cols, m, n, k, epi, act, L.ptr(bias), L.ptr(aux), aux.stride(0) if aux is not None else 0,
            alpha, L.ptr(ws), ws_bytes, L.stream())
    if matmul is None:
        L.check(lib.bsig_gemm_f32(*args))
    else:
        if matmul == 1:      # the new kernel runs this call
            gathered = int(a_rows is not None or b_rows is not None)
            assert _path(B, m, n, k, a_km, b_km, gathered, epi, ws_bytes)[0] == L.GEMM_PATH_SPLIT_BF16
        L.check(lib.bsig_gemm_f32_ex(*args, matmul))
    return c


def _operand(logical, kmajor, gather, gen):
    """Device storage of the logical [rows, k] operand: k-contiguous or k-major, directly or through an
    index vector with repeated and out-of-order entries into a larger, shuffled storage (of the rows of a
    k-contiguous operand, of the contraction index of a k-major one -- what GemmParams gathers)."""
    mat = logical.T.contiguous() if kmajor else logical.contiguous()       # [gathered dim, other]
    if not gather:
        return mat.to(DEV), None
    g = mat.shape[0]
    perm = torch.randperm(g + 3, generator=gen)
    rows = perm[:g].clone()                       # where logical row i lives
    store = torch.randn(g + 3, mat.shape[1], generator=gen).to(mat.dtype)
    store[rows] = mat
    if g > 2:                                     # a repeated entry: rows 0 and g - 1 are the same source row
        mat2 = mat.clone()
        mat2[g - 1] = mat[0]
        rows[g - 1] = rows[0]
        logical.copy_(mat2.T if kmajor else mat2)
    return store.to(DEV), rows.to(torch.int32).to(DEV)


def _slab_variants(m, n, k):
    """workspaces in [m, n] slabs: one that forces 1 slice and one that allows >= 2 where k is long enough"""
    if (m, n, k) == BIG:
        return [1, 2]
    return [None] if k < 1040 else [1, 64]


def _tile(B, m, n, k):
    return _path(B, m, n, k, 0, 0, 0, 0, 0)[1]


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize('a_km,b_km', LAYOUTS)
@pytest.mark.parametrize('m,n,k', SHAPES)
def test_small_integers_are_exact(B, m, n, k, a_km, b_km):
    """Integers in [-8, 8] are bf16-exact (p1 = p2 = 0) and every partial sum is below 2^24: the result is
    the integer product."""
    for gather in (False, True):
        for slabs in _slab_variants(m, n, k):
            gen = torch.Generator().manual_seed(m + n + k + gather)
            a_t = torch.randint(-8, 9, (m, k), generator=gen).float()
            b_t = torch.randint(-8, 9, (n, k), generator=gen).float()
            a, a_rows = _operand(a_t, a_km, gather, gen)
            b, b_rows = _operand(b_t, b_km, gather, gen)
            want = (a_t.double() @ b_t.double().T).float()
            assert _tile(B, m, n, k) == (128 if (m, n, k) == BIG else 64)
            if slabs is not None:
                sl = _path(B, m, n, k, a_km, b_km, int(gather), 0, slabs * 4 * m * n)[3]
                assert sl == 1 if slabs == 1 else (sl >= 2 and k % _path(B, m, n, k, a_km, b_km, int(gather), 0,
                                                                        slabs * 4 * m * n)[4] != 0)
            got = _gemm(B, a, b, m, n, k, a_km, b_km, 1, a_rows=a_rows, b_rows=b_rows, slabs=slabs).cpu()
            assert torch.equal(got, want), (gather, slabs)


def _full_mantissa(shape, gen):
    """fp32 values with 24 random mantissa bits, a random sign and an exponent in [-100, 100]"""
    mant = torch.randint(1 << 23, 1 << 24, shape, generator=gen).double()
    expo = torch.randint(-100, 101, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    x = (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo - 23)).float()
    assert torch.isfinite(x).all() and (x != 0).all()
    return x


@pytest.mark.parametrize('a_km,b_km', LAYOUTS)
@pytest.mark.parametrize('m,n,k', SHAPES)
def test_selection_returns_every_bit(B, m, n, k, a_km, b_km):
    """A with full 24-bit mantissas against a 0/1 selection matrix: C is the selected entries of A bit for
    bit -- a lost or misplaced piece (p2 is 2^-16 of the element) fails here."""
    for gather in (False, True):
        for slabs in _slab_variants(m, n, k):
            gen = torch.Generator().manual_seed(7 * m + n + k + gather)
            a_t = _full_mantissa((m, k), gen)
            sel = torch.randint(0, k, (n,), generator=gen)
            b_t = torch.zeros(n, k)
            b_t[torch.arange(n), sel] = 1.0
            a, a_rows = _operand(a_t, a_km, gather, gen)
            b, _ = _operand(b_t, b_km, False, gen)
            got = _gemm(B, a, b, m, n, k, a_km, b_km, 1, a_rows=a_rows, slabs=slabs).cpu()
            assert torch.equal(got.view(torch.int32), a_t[:, sel].contiguous().view(torch.int32)), (gather, slabs)
            # and the mirror image: B carries the mantissas
            b2_t = _full_mantissa((n, k), gen)
            sel_m = torch.randint(0, k, (m,), generator=gen)
            a2_t = torch.zeros(m, k)
            a2_t[torch.arange(m), sel_m] = 1.0
            a2, _ = _operand(a2_t, a_km, False, gen)
            b2, b2_rows = _operand(b2_t, b_km, gather, gen)
            got = _gemm(B, a2, b2, m, n, k, a_km, b_km, 1, b_rows=b2_rows, slabs=slabs).cpu()
            assert torch.equal(got.view(torch.int32), b2_t[:, sel_m].T.contiguous().view(torch.int32)), (gather, slabs)


# ---------------------------------------------------------------------- error
RATIOS = {}


@pytest.mark.parametrize('dist', ['normal', 'positive'])
@pytest.mark.parametrize('a_km,b_km', LAYOUTS)
@pytest.mark.parametrize('m,n,k', SHAPES)
def test_error_against_fp64(B, m, n, k, a_km, b_km, dist):
    gen = torch.Generator().manual_seed(3 * m + 5 * n + k)
    draw = (lambda *s: torch.randn(*s, generator=gen)) if dist == 'normal' else \
        (lambda *s: torch.rand(*s, generator=gen) + 0.01)
    a_t, b_t = draw(m, k), draw(n, k)
    a, _ = _operand(a_t, a_km, False, gen)
    b, _ = _operand(b_t, b_km, False, gen)
    ref = a_t.double() @ b_t.double().T
    mag = a_t.double().abs() @ b_t.double().abs().T
    for slabs in _slab_variants(m, n, k):
        # the yardstick: the fp32 kernel on the same inputs, the workspace included (its K slices shorten
        # its chains as they do the new kernel's)
        fp32 = _gemm(B, a, b, m, n, k, a_km, b_km, None, slabs=slabs).cpu()
        got = _gemm(B, a, b, m, n, k, a_km, b_km, 1, slabs=slabs).cpu()
        again = _gemm(B, a, b, m, n, k, a_km, b_km, 1, slabs=slabs).cpu()
        err = (got.double() - ref).abs()
        # 1. the derived guard
        assert (err <= ((6 * k + 8) * U23 + U23) * mag).all(), float((err / mag).max() / U23)
        # 2. the sharp criterion: no worse than twice the fp32 kernel on the same inputs
        rel = float((err / mag).max())
        rel32 = float(((fp32.double() - ref).abs() / mag).max())
        RATIOS[(m, n, k, a_km, b_km, dist, slabs)] = rel / max(rel32, 1e-300)
        print('split-bf16 error %.2f u, fp32 kernel %.2f u, ratio %.2f  %s' % (
            rel * 2 ** 24, rel32 * 2 ** 24, rel / max(rel32, 1e-300), (m, n, k, a_km, b_km, dist, slabs)))
        if k >= 257:
            assert rel <= 2.0 * rel32, (rel * 2 ** 24, rel32 * 2 ** 24)
        # 3. the new arithmetic ran, and it is reproducible
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        if k >= 50:
            assert not torch.equal(got, fp32)
        # matmul = 0 through the new entry point is the fp32 kernel, bit for bit
        assert torch.equal(_gemm(B, a, b, m, n, k, a_km, b_km, 0, slabs=slabs).cpu().view(torch.int32),
                           fp32.view(torch.int32))


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('a_km,b_km', LAYOUTS)
def test_nonfinite_operand_element(B, a_km, b_km, bad):
    m, n, k = 130, 70, 257
    gen = torch.Generator().manual_seed(11)
    a_t, b_t = torch.randn(m, k, generator=gen), torch.randn(n, k, generator=gen)
    a_t[37, 200] = bad
    b_t[5, 256] = bad
    a, _ = _operand(a_t, a_km, False, gen)
    b, _ = _operand(b_t, b_km, False, gen)
    got = _gemm(B, a, b, m, n, k, a_km, b_km, 1).cpu()
    hit = torch.zeros(m, n, dtype=torch.bool)
    hit[37, :] = True
    hit[:, 5] = True
    assert not torch.isfinite(got[hit]).any() and torch.isfinite(got[~hit]).all()


# ------------------------------------------------------------------ epilogues
@pytest.mark.parametrize('a_km,b_km', LAYOUTS)
@pytest.mark.parametrize('epi', ['bias', 'bias_tanh', 'bias_relu', 'cos_sin', 'cos_off', 'mul_dact'])
def test_epilogues(B, epi, a_km, b_km):
    """Every epilogue at (130, 70, 257) against fp64: the guard g on the accumulator, pushed through the
    epilogue's Lipschitz constant Lip, plus the fp32 evaluation of the epilogue itself -- the rounding of
    its argument (2^-24 |arg| Lip) and of its result (4 u |out|: sincosf / tanhf are within a few ulp)."""
    L = B._lib
    m, n, k = 130, 70, 257
    gen = torch.Generator().manual_seed(23)
    a_t, b_t = torch.randn(m, k, generator=gen) * 0.3, torch.randn(n, k, generator=gen) * 0.3
    bias_t, aux_t = torch.randn(n, generator=gen), torch.tanh(torch.randn(m, n, generator=gen))
    a, _ = _operand(a_t, a_km, False, gen)
    b, _ = _operand(b_t, b_km, False, gen)
    pre = a_t.double() @ b_t.double().T
    g = ((6 * k + 8) * U23 + U23) * (a_t.double().abs() @ b_t.double().abs().T)
    bias, aux, alpha = bias_t.to(DEV), aux_t.to(DEV), 0.25
    bd = bias_t.double()
    if epi == 'bias':
        kw, want, lip, arg = dict(epi=L.EPI_BIAS, bias=bias), pre + bd, 1.0, pre + bd
    elif epi == 'bias_tanh':
        kw, want, lip, arg = dict(epi=L.EPI_BIAS_ACT, act=L.ACT_TANH, bias=bias), torch.tanh(pre + bd), 1.0, pre + bd
    elif epi == 'bias_relu':
        kw, want, lip, arg = dict(epi=L.EPI_BIAS_ACT, act=L.ACT_RELU, bias=bias), torch.relu(pre + bd), 1.0, pre + bd
    elif epi == 'cos_sin':
        kw, want, lip, arg = dict(epi=L.EPI_COS_SIN, alpha=alpha), \
            alpha * torch.cat([torch.cos(pre), torch.sin(pre)], 1), alpha, torch.cat([pre, pre], 1)
        g = torch.cat([g, g], 1)
    elif epi == 'cos_off':
        kw, want, lip, arg = dict(epi=L.EPI_COS_OFF, bias=bias, alpha=alpha), alpha * torch.cos(pre + bd), alpha, pre + bd
    else:
        kw, want, lip, arg = dict(epi=L.EPI_MUL_DACT, act=L.ACT_TANH, aux=aux), pre * (1 - aux_t.double() ** 2), 1.0, pre
    bound = lip * (g + 2.0 ** -24 * arg.abs()) + 4 * 2.0 ** -24 * want.abs() + 1e-30
    # no workspace: one slice, the kernel's own fused epilogue; the default one: 2 slices, gemm_reduce_kernel's
    for slabs, slices in ((0, 1), (None, 2)):
        ws_bytes = 0 if slabs == 0 else int(B._lib.load().bsig_gemm_workspace_bytes(m, n, k))
        assert _path(B, m, n, k, a_km, b_km, 0, kw['epi'], ws_bytes)[3] == slices
        got = _gemm(B, a, b, m, n, k, a_km, b_km, 1, slabs=slabs, **kw).cpu().double()
        assert got.shape == want.shape and (got - want).abs().le(bound).all(), \
            (slabs, float(((got - want).abs() / bound).max()))
        fp32 = _gemm(B, a, b, m, n, k, a_km, b_km, None, slabs=slabs, **kw).cpu().double()
        assert not torch.equal(got, fp32)


# ------------------------------------------------------------------------ RFF
RFF_VARIANTS = ['cos_rbf'] + ['%s.%s' % (k, m) for k in ('Matern12', 'Matern32', 'Matern52', 'Laplace')
                              for m in ('cossin', 'cos')]


@pytest.mark.parametrize('tag', RFF_VARIANTS)
def test_rff_variants_match_reference(B, tag):
    """bsig_rff_project_ex(matmul = 1) on the cases of tests/golden/rff_variants.npz at the project's own
    tolerance for HIP features, 3e-6 max(1, |inner| / 8), against the reference's features and the fp64 map."""
    g = golden('rff_variants.npz')
    if tag == 'cos_rbf':
        args, xk = dict(n_feat=64, d=302, sigma=4.0, cos_only=True, kernel='RBF'), 'x'
    else:
        kern, mode = tag.split('.')
        args, xk = dict(n_feat=48, d=150, sigma=[0.5 + 0.01 * j for j in range(150)],
                        cos_only=(mode == 'cos'), kernel=kern), 'x150'
    np.random.seed(int(g[tag + '.seed']))
    rff = B.RFF(quasi_random=False, device=DEV, **args)
    np.testing.assert_array_equal(rff.freqs.cpu().numpy(), g[tag + '.freqs'])
    x = torch.from_numpy(g[xk]).to(DEV)
    assert rff.matmul_precision == 'float32'
    plain = rff.to_features(x).cpu().numpy()
    rff.matmul_precision = 'split_bf16'
    mf = rff.m_feat
    assert _path(B, x.shape[0], mf, args['d'], 0, 0, 0, B._lib.EPI_COS_OFF if args['cos_only'] else B._lib.EPI_COS_SIN,
                 int(B._lib.load().bsig_gemm_workspace_bytes(x.shape[0], mf, args['d'])))[0] == B._lib.GEMM_PATH_SPLIT_BF16
    out = rff.to_features(x).cpu().numpy()
    assert out.shape == g[tag + '.features'].shape and not np.array_equal(out, plain)
    sig = rff.sigma.cpu().numpy().astype(np.float64)
    inner = g[xk].astype(np.float64) @ (g[tag + '.freqs'].astype(np.float64) / sig).T
    if not args['cos_only']:
        inner = np.concatenate([inner, inner], axis=1)
    tol = 3e-6 * np.maximum(1.0, np.abs(inner) / 8.0)
    err = np.abs(out - g[tag + '.features'])
    assert (err <= tol).all(), (tag, float((err / tol).max()))
    if args['cos_only']:
        f64 = float(g[tag + '.a']) * np.cos(inner + g[tag + '.offset'].astype(np.float64))
    else:
        half = inner[:, :inner.shape[1] // 2]
        f64 = float(g[tag + '.a']) * np.concatenate([np.cos(half), np.sin(half)], axis=1)
    assert (np.abs(out - f64) <= tol).all()


# ----------------------------------------------------------------------- fits
def _run_chunk(B, tag, g, summ, theta, precision):
    from test_gpu_fit import _chunk_model
    m = _chunk_model(B, tag, g, summ.shape[1])
    assert m.matmul_precision == 'float32'
    m.set_matmul_precision(precision)
    logs = m.run_training(summ, theta, int(g['n_updates']), int(g['batch']), ids_table=g['ids'])
    assert m._plan is not None and int(m._prec.is_persistent(m._plan)) == 0       # the per-phase kernels ran
    return m, logs


@pytest.mark.parametrize('tag', ['mdnn_start', 'mdnn_corrdiff_full', 'mdrff_corrdiff', 'mdrff_matern32'])
@pytest.mark.parametrize('use_graph', [True, False])
def test_teacher_forced_chunk_matches_reference(B, tag, use_graph, monkeypatch):
    """The four reference chunks with set_matmul_precision('split_bf16') on the per-phase kernels
    (BSIG_NO_PERSISTENT=1, set and restored here: the persistent kernels compute in fp32 and are not
    touched by the mode): the assertions and tolerances of tests/test_gpu_fit.py's test of the same name."""
    from test_gpu_fit import CHUNKS
    monkeypatch.setenv('BSIG_NO_PERSISTENT', '1')
    g = golden('chunk_%s.npz' % tag)
    B.MDNN.EPS_NOISE = 0.0
    B.MDNN.USE_GRAPH = use_graph
    states = torch.from_numpy(g['states']).to(DEV)
    actions = torch.from_numpy(g['actions']).to(DEV)
    theta = torch.from_numpy(g['theta']).to(DEV)
    summ = getattr(B.summarizers, CHUNKS[tag]['summarizer'])(states, actions)
    m, logs = _run_chunk(B, tag, g, summ, theta, 'split_bf16')
    print(tag, use_graph, 'max rel diff of the logs against the reference: %.3g' % max(
        abs(a - b) / max(abs(b), 1e-12) for key in ('train_loss', 'test_loss') for a, b in zip(logs[key], g[key])))
    np.testing.assert_allclose(logs['test_loss'], g['test_loss'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(logs['train_loss'], g['train_loss'], rtol=1e-4, atol=1e-5)
    n_train = int(states.shape[0] * 0.8)
    mog = m.predict_MoGs(summ[n_train:n_train + 1])[0]
    np.testing.assert_allclose(mog.a, g['mog.a'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(np.stack([c.m for c in mog.xs]), g['mog.ms'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.stack([c.S for c in mog.xs]), g['mog.Ss'], rtol=1e-4, atol=1e-7)
    nll = -mog.eval(g['theta'][n_train:n_train + 1].astype(np.float64), log=True)
    np.testing.assert_allclose(nll, g['mog.nll_true'], rtol=1e-4, atol=1e-5)
    # the new arithmetic ran: the 6 + 6 logs are not bitwise those of the same run in float32
    _, plain = _run_chunk(B, tag, g, summ, theta, 'float32')
    assert len(logs['train_loss']) == 6 and len(logs['test_loss']) == 6
    assert (list(logs['train_loss']), list(logs['test_loss'])) != (list(plain['train_loss']), list(plain['test_loss']))
    # and reproducible: the same run again gives the same logs bit for bit
    _, again = _run_chunk(B, tag, g, summ, theta, 'split_bf16')
    assert again == logs


def test_the_mode_does_not_change_the_engine(B):
    """Without BSIG_NO_PERSISTENT the plan of a chunk picks the engine it picks in float32; where that is a
    persistent update kernel (which computes in fp32 and is not touched by the mode) and nothing of the call
    goes through the GEMM dispatch -- an MDNN --, the logs are bitwise the float32 run's."""
    from test_gpu_fit import CHUNKS, _chunk_model
    assert os.environ.get('BSIG_NO_PERSISTENT') != '1'
    B.MDNN.EPS_NOISE = 0.0
    for tag in ('mdnn_start', 'mdrff_corrdiff'):
        g = golden('chunk_%s.npz' % tag)
        summ = getattr(B.summarizers, CHUNKS[tag]['summarizer'])(torch.from_numpy(g['states']).to(DEV),
                                                                   torch.from_numpy(g['actions']).to(DEV))
        theta = torch.from_numpy(g['theta']).to(DEV)
        out = {}
        for precision in ('float32', 'split_bf16'):
            m = _chunk_model(B, tag, g, summ.shape[1]).set_matmul_precision(precision)
            logs = m.run_training(summ, theta, int(g['n_updates']), int(g['batch']), ids_table=g['ids'])
            out[precision] = (int(m._prec.is_persistent(m._plan)), logs)
        assert out['float32'][0] == out['split_bf16'][0], tag
        if out['float32'][0] and CHUNKS[tag]['cls'] == 'MDNN':
            # (an MDRFF's feature cache is projected through the GEMM dispatch whatever the engine: its logs move)
            assert out['float32'][1] == out['split_bf16'][1], tag
        np.testing.assert_allclose(out['split_bf16'][1]['test_loss'], g['test_loss'], rtol=1e-4, atol=1e-5)


def test_large_minibatch_against_the_oracle(B, monkeypatch):
    """bench.scaled_nll_check under BSIG_MATMUL_PRECISION=split_bf16 on cfg2: 3000 synthetic pairs, minibatch
    2048, 4 updates, teacher-forced against the oracle."""
    import bench
    L, lib = B._lib, B._lib.load()
    cfg = bench.CONFIGS['cfg2']
    monkeypatch.setenv('BSIG_MATMUL_PRECISION', 'split_bf16')
    monkeypatch.setenv('BSIG_NO_PERSISTENT', '1')
    theta, states, actions = bench.synth_pairs(cfg, 3000, 5, DEV)
    res = bench.scaled_nll_check(B, cfg, theta, states, actions, DEV, 2048, n=3000, n_updates=4)
    print('large minibatch, split_bf16: max_rel_diff_all_logs = %.3g' % res['max_rel_diff_all_logs'])
    assert res['max_rel_diff_all_logs'] < 1e-4, res
    model = bench.build_gpu_model(B, cfg, DEV, 78).model
    assert model.matmul_precision == 'split_bf16' and model.rff.matmul_precision == 'split_bf16'
    nh = int(lib.bsig_head_width(C.byref(model._cfg().head)))
    nf, mf, d_in, batch = model.rff.n_feat, model.rff.m_feat, model.input_dim, 2048
    ws = lambda m, n, k: int(lib.bsig_gemm_workspace_bytes(m, n, k))
    assert _path(B, batch, nh, nf, 0, 0, 1, L.EPI_BIAS, ws(batch, nh, nf))[0] == L.GEMM_PATH_SPLIT_BF16       # head forward
    assert _path(B, nh, nf, batch, 1, 1, 1, 100, ws(nh, nf, batch))[0] == L.GEMM_PATH_SPLIT_BF16             # head gradient + Adam
    assert _path(B, 3000, mf, d_in, 0, 0, 0, L.EPI_COS_SIN, ws(3000, mf, d_in))[0] == L.GEMM_PATH_SPLIT_BF16  # projection
