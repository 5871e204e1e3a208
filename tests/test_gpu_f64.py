"""GPU checks of the fp64 mode (include/bsig_f64.h, MDNN.double()): every op through the C ABI
against numpy / the oracle in float64, one-step gradients and Adam, teacher-forced chunks against
the oracle under torch.set_default_dtype(torch.float64), BayesSim, determinism and flags.

Tolerances.  GEMM: the standard summation bound (K + 2) 2^-53 (|A| |B|).  Head, gradients, Adam:
1e-12 of each array's largest magnitude (an output costs at most about 10^3 double operations at
1.1e-16).  Chunks: no fixed number -- the fp64 oracle is run in eight input-column orders and the
device run must sit within 8 x their spread + 1e-11 |ref|, where that spread itself is <= 1e-8."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden
import head_cases as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -53


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


@pytest.fixture(autouse=True)
def _eps_guard():
    import bayes_sim_ig_amd as pkg
    old = pkg.MDNN.EPS_NOISE
    yield
    pkg.MDNN.EPS_NOISE = old


@contextlib.contextmanager
def default_f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def _close(got, ref, tol=1e-12, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-300)
    err = np.abs(got - ref).max() / scale
    print('%s: max |err| / max |ref| = %.3g' % (what, err))
    assert err <= tol, (what, err)


# ------------------------------------------------------------------ GEMM
def _gemm(B, a, b, m, n, k, a_km=0, b_km=0, a_rows=None, b_rows=None, epi=0, act=0, bias=None, aux=None,
          alpha=1.0, ldc=None):
    _lib = B._lib
    lib = _lib.load()
    ta, tb = _dev(a), _dev(b)
    ldc = ldc or (2 * n if epi == _lib.EPI_COS_SIN else n)
    out = torch.zeros(m, ldc, dtype=torch.float64, device=DEV)
    tr_a, tr_b = _dev(a_rows, torch.int32), _dev(b_rows, torch.int32)
    tbias, taux = _dev(bias), _dev(aux)
    _lib.check(lib.bsig_gemm_f64(_lib.ptr(ta), ta.stride(0), a_km, _lib.ptr(tr_a), _lib.ptr(tb), tb.stride(0),
                                 b_km, _lib.ptr(tr_b), _lib.ptr(out), ldc, m, n, k, epi, act, _lib.ptr(tbias),
                                 _lib.ptr(taux), taux.stride(0) if taux is not None else 0, alpha,
                                 _lib.stream()))
    return out.cpu().numpy()


def _bound_ok(got, ref, absprod, k, what):
    worst = (np.abs(got - ref) / ((k + 2) * U * absprod + 1e-300)).max()
    print('%s: worst |err| / bound = %.3g' % (what, worst))
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize('m,n,k', [(100, 128, 40), (100, 33, 1), (7, 260, 130)])
def test_gemm_k_contiguous(B, m, n, k):
    r = np.random.RandomState(m + n + k)
    a, b = r.randn(m, k), r.randn(n, k)
    got = _gemm(B, a, b, m, n, k)
    _bound_ok(got, a @ b.T, np.abs(a) @ np.abs(b).T, k, 'k-contiguous')
    assert np.array_equal(got, _gemm(B, a, b, m, n, k))          # two runs bitwise equal


def test_gemm_row_gather_with_repeated_ids(B):
    r = np.random.RandomState(1)
    src, w = r.randn(250, 40), r.randn(128, 40)
    ids = r.randint(0, 250, 100)
    ids[:4] = ids[4]
    got = _gemm(B, src, w, 100, 128, 40, a_rows=ids)
    _bound_ok(got, src[ids] @ w.T, np.abs(src[ids]) @ np.abs(w).T, 40, 'gather')


def test_gemm_k_major_weight_gradient_shape(B):
    """dW = dO^T X at K = 4, D = 4, B = 100: both operands k-major, the long one gathered."""
    r = np.random.RandomState(2)
    d_o, x = r.randn(100, 36), r.randn(250, 130)
    ids = r.randint(0, 250, 100)
    got = _gemm(B, d_o, x, 36, 130, 100, a_km=1, b_km=1, b_rows=ids)
    _bound_ok(got, d_o.T @ x[ids], np.abs(d_o).T @ np.abs(x[ids]), 100, 'k-major')
    assert np.array_equal(got, _gemm(B, d_o, x, 36, 130, 100, a_km=1, b_km=1, b_rows=ids))


def test_gemm_every_epilogue(B):
    L = B._lib
    m, n, k = 100, 128, 40
    r = np.random.RandomState(3)
    a, b, bias = r.randn(m, k) * 0.3, r.randn(n, k) * 0.3, r.randn(n)
    acc = a @ b.T
    # the product itself obeys the summation bound; an epilogue adds a few roundings of its own value
    eps_epi = lambda ref: 8 * U * (np.abs(ref) + 1.0) + (k + 2) * U * (np.abs(a) @ np.abs(b).T)
    def check(got, ref, what):
        worst = (np.abs(got - ref) / eps_epi(ref)).max()
        print('%s: worst |err| / bound = %.3g' % (what, worst))
        assert worst <= 1.0, what
    check(_gemm(B, a, b, m, n, k, epi=L.EPI_NONE), acc, 'none')
    check(_gemm(B, a, b, m, n, k, epi=L.EPI_BIAS, bias=bias), acc + bias, 'bias')
    z = acc + bias
    acts = {L.ACT_TANH: np.tanh(z), L.ACT_RELU: np.maximum(z, 0), L.ACT_LEAKY_RELU: np.where(z > 0, z, 0.01 * z),
            L.ACT_SIGMOID: 1 / (1 + np.exp(-z)), L.ACT_IDENTITY: z}
    for act, ref in acts.items():
        check(_gemm(B, a, b, m, n, k, epi=L.EPI_BIAS_ACT, act=act, bias=bias), ref, 'bias_act %d' % act)
    h = {L.ACT_TANH: np.tanh(z), L.ACT_RELU: np.maximum(z, 0), L.ACT_LEAKY_RELU: np.where(z > 0, z, 0.01 * z),
         L.ACT_SIGMOID: 1 / (1 + np.exp(-z)), L.ACT_IDENTITY: z}
    dact = {L.ACT_TANH: lambda v: 1 - v * v, L.ACT_RELU: lambda v: (v > 0) * 1.0,
            L.ACT_LEAKY_RELU: lambda v: np.where(v > 0, 1.0, 0.01), L.ACT_SIGMOID: lambda v: v * (1 - v),
            L.ACT_IDENTITY: lambda v: np.ones_like(v)}
    for act in acts:
        check(_gemm(B, a, b, m, n, k, epi=L.EPI_MUL_DACT, act=act, aux=h[act]), acc * dact[act](h[act]),
              'mul_dact %d' % act)


def test_rff_map_in_double(B):
    L = B._lib
    lib = L.load()
    r = np.random.RandomState(4)
    rows, i_dim, nf = 100, 302, 24
    x, co, off = r.randn(rows, i_dim) * 0.2, r.randn(nf, i_dim) * 0.25, r.rand(nf) * 2 * np.pi
    a = np.sqrt(1.0 / nf)
    inner = x @ co.T
    bound = (i_dim + 2) * U * (np.abs(x) @ np.abs(co).T) + 8 * U      # |d cos| <= |d inner|, a < 1
    tx, tc, to = _dev(x), _dev(co), _dev(off)
    for cos_only in (0, 1):
        feats = torch.zeros(rows, nf if cos_only else 2 * nf, dtype=torch.float64, device=DEV)
        L.check(lib.bsig_rff_project_f64(L.ptr(tx), i_dim, None, L.ptr(tc), i_dim, L.ptr(to) if cos_only else None,
                                         L.ptr(feats), feats.stride(0), rows, i_dim, nf, a, cos_only, L.stream()))
        ref = a * np.cos(inner + off) if cos_only else a * np.concatenate([np.cos(inner), np.sin(inner)], 1)
        got = feats.cpu().numpy()
        worst = (np.abs(got - ref) / np.concatenate([bound] * (1 if cos_only else 2), 1)).max()
        print('rff cos_only=%d: worst |err| / bound = %.3g' % (cos_only, worst))
        assert worst <= 1.0


# ------------------------------------------------------------------ head
def _hyper(B, eps):
    return B._lib.F64Hyper(1e-3, 0.9, 0.999, 1e-8, eps, 1e-5, 1e5, 0.0)


def _head_dims(B, d, k, full, eps):
    dims = B._lib.HeadDims()
    dims.out_dim, dims.n_comp, dims.full_cov = d, k, int(full)
    dims.eps_noise, dims.min_weight, dims.ll_limit = eps, 1e-5, 1e5
    return dims


HEAD_CASES = [(9, 3, 4, False), (7, 2, 10, False), (5, 1, 1, False), (9, 4, 3, True), (9, 5, 3, True),
              (33, 13, 10, False), (7, 49, 10, False), (7, 32, 10, True), (5, 8, 64, False)]
# (batch, D, K, full).  The fp64 head has ONE path (a wavefront per row, four rows per workgroup, a single-slab
# finish), so the 27 shapes of tests/head_cases.py -- which walk the fp32 head's four paths and its slab
# thresholds -- reduce to these: their extreme D / K of either covariance, plus the issue's D = 3 / K = 4 and
# full-covariance D = 4 / K = 3, at batches that are no multiple of four.


@pytest.mark.parametrize('eps', [0.0, 1e-5])
@pytest.mark.parametrize('b,d,k,full,clamp', [c + (cl,) for c in HEAD_CASES for cl in (False, True)
                                              if not (cl and c[2] == 1)])   # (K = 1 has nothing to clamp)
def test_head_nll_and_grad_match_closed_form(B, b, d, k, full, clamp, eps):
    from oracle.estimators import mdn_head_closed_form
    L = B._lib
    lib = L.load()
    r = np.random.RandomState(b * 1000 + d * 10 + k)
    ls = d * (d - 1) // 2 if full else 0
    nh = k + 2 * d * k + ls * k
    o = r.randn(b, nh) * 0.5
    if clamp:          # one dominant logit: the other softmax weights fall below MIN_WEIGHT
        o[:, 0] += 25.0
    y = r.rand(b, d)
    noise = r.rand(b, d, k) if eps else None
    loss_ref, d_ref, _ = mdn_head_closed_form(o, y, d, k, full, eps_noise=eps, noise=noise)
    dims = _head_dims(B, d, k, full, eps)
    to, ty, tn = _dev(o), _dev(y), _dev(noise)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    d_o = torch.full((b, nh), float('nan'), dtype=torch.float64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.bsig_head_workspace_bytes_f64(C.byref(dims), b)) // 8 + 1, dtype=torch.float64,
                     device=DEV)
    L.check(lib.bsig_mdn_head_nll_f64(C.byref(dims), C.byref(_hyper(B, eps)), L.ptr(to), nh, L.ptr(ty), d, None,
                                      b, b, L.ptr(tn), 0, 0, L.ptr(loss), L.ptr(d_o), L.ptr(flag), L.ptr(ws),
                                      ws.numel() * 8, L.stream()))
    assert int(flag.item()) == 0
    assert abs(float(loss.item()) - loss_ref) <= 1e-12 * abs(loss_ref)
    _close(d_o.cpu().numpy(), d_ref, 1e-12, 'dO')


def test_head_philox_jitter_is_the_fp32_draw_widened(B):
    """Without injected noise the jitter is the uniform of the fp32 thread-per-component kernels."""
    from oracle.estimators import mdn_head_closed_form
    L = B._lib
    lib = L.load()
    b, d, k, eps, seed, sid = 6, 3, 4, 1e-2, 1234567, 5
    r = np.random.RandomState(0)
    nh = k + 2 * d * k
    o, y = r.randn(b, nh) * 0.5, r.rand(b, d)
    u = H.draws_flat(b, d, k, seed, sid)
    loss_ref, d_ref, _ = mdn_head_closed_form(o, y, d, k, False, eps_noise=eps, noise=u)
    dims = _head_dims(B, d, k, False, eps)
    to, ty = _dev(o), _dev(y)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    d_o = torch.zeros(b, nh, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.bsig_head_workspace_bytes_f64(C.byref(dims), b)) // 8 + 1, dtype=torch.float64,
                     device=DEV)
    L.check(lib.bsig_mdn_head_nll_f64(C.byref(dims), C.byref(_hyper(B, eps)), L.ptr(to), nh, L.ptr(ty), d, None,
                                      b, b, None, seed, sid, L.ptr(loss), L.ptr(d_o), None, L.ptr(ws),
                                      ws.numel() * 8, L.stream()))
    assert abs(float(loss.item()) - loss_ref) <= 1e-12 * abs(loss_ref)
    _close(d_o.cpu().numpy(), d_ref, 1e-12, 'dO (Philox)')


@pytest.mark.parametrize('eps', [0.0, 1e-5])
@pytest.mark.parametrize('b,d,k,full', [(5, 3, 4, False), (9, 4, 3, True)])
def test_head_outputs_and_tuple_loss_match_closed_form(B, b, d, k, full, eps):
    """bsig_mdn_head_outputs_f64 (weights, mu, L_d, lower; injected noise) and bsig_mdn_nll_from_tuple_f64 of that
    tuple, called directly, against the closed form; the flag word stays clear, and a NaN in one mu raises it."""
    from oracle.estimators import mdn_head_closed_form
    L = B._lib
    lib = L.load()
    r = np.random.RandomState(b * 100 + d * 10 + k)
    ls = d * (d - 1) // 2 if full else 0
    nh = k + 2 * d * k + ls * k
    o, y, noise = r.randn(b, nh) * 0.5, r.rand(b, d), r.rand(b, d, k)
    loss_ref, _, aux = mdn_head_closed_form(o, y, d, k, full, eps_noise=eps, noise=noise)
    dims, hy = _head_dims(B, d, k, full, eps), _hyper(B, eps)
    to, ty, tn = _dev(o), _dev(y), _dev(noise)
    outs = [torch.full((b, n), float('nan'), dtype=torch.float64, device=DEV) for n in (k, d * k, d * k, max(ls * k, 1))]
    loss = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.bsig_head_workspace_bytes_f64(C.byref(dims), b)) // 8 + 1, dtype=torch.float64,
                     device=DEV)

    def outputs(src):
        L.check(lib.bsig_mdn_head_outputs_f64(C.byref(dims), C.byref(hy), L.ptr(src), nh, b, L.ptr(tn), 0, 0,
                                              L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]),
                                              L.ptr(outs[3]) if full else None, L.ptr(flag), L.ptr(ws), ws.numel() * 8,
                                              L.stream()))

    def tuple_loss():
        L.check(lib.bsig_mdn_nll_from_tuple_f64(C.byref(dims), C.byref(hy), L.ptr(outs[0]), L.ptr(outs[1]),
                                                L.ptr(outs[2]), L.ptr(outs[3]) if full else None, L.ptr(ty), d, b,
                                                L.ptr(loss), L.ptr(flag), L.ptr(ws), ws.numel() * 8, L.stream()))
    outputs(to)
    tuple_loss()
    assert int(flag.item()) == 0
    for got, key in zip(outs[:4 if full else 3], ('weights', 'mu', 'l_d', 'lower')):
        _close(got.cpu().numpy(), np.asarray(aux[key]).reshape(b, -1), 1e-12, key)
    assert abs(float(loss.item()) - loss_ref) <= 1e-12 * abs(loss_ref)
    o[b - 1, k + d * k - 1] = np.nan
    outputs(_dev(o))
    assert int(flag.item()) == 1
    flag.zero_()
    tuple_loss()                      # (the tuple now carries the NaN)
    assert int(flag.item()) == 1


# ------------------------------------------------------------------ one step
STEP_CFG = {
    'diag': dict(cls='MDNN', input_dim=40, output_dim=2, n_gaussians=10, full_covariance=False,
                 hidden_layers=(24, 24), lr=5e-4),
    'full': dict(cls='MDNN', input_dim=12, output_dim=5, n_gaussians=3, full_covariance=True,
                 hidden_layers=(16,), lr=1e-3),
    'mdrff': dict(cls='MDRFF', input_dim=302, output_dim=13, n_gaussians=4, full_covariance=False, lr=1e-3,
                  n_feat=64, sigma=4.0),
    'clamp': dict(cls='MDNN', input_dim=6, output_dim=3, n_gaussians=5, full_covariance=False,
                  hidden_layers=(8,), lr=1e-3),
}


def _w0(g):
    return {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('w0.')}


def _double_oracle_rff(o):
    o.rff.freqs, o.rff.sigma = o.rff.freqs.double(), o.rff.sigma.double()


@pytest.mark.parametrize('tag', ['diag_eps0', 'full_eps1e5', 'clamp_eps1e5', 'mdrff_eps0', 'mdrff_eps1e5'])
def test_one_step_grads_and_adam(B, tag):
    from oracle import estimators as oest
    g = golden('mdn_step_%s.npz' % tag)
    kw = dict(STEP_CFG[tag.split('_')[0]])
    cls = kw.pop('cls')
    d = kw['output_dim']
    B.MDNN.EPS_NOISE = float(g['eps_noise'])
    kw.update(output_lows=np.zeros(d), output_highs=np.ones(d), activation=torch.nn.Tanh)
    extra = dict(freqs=g['rff.freqs']) if cls == 'MDRFF' else {}
    m = getattr(B, cls)(device=DEV, **extra, **kw)
    m.load_state_dict(_w0(g))
    m.double()
    x, y, noise = (torch.from_numpy(g[n]) for n in ('x', 'y', 'noise'))
    loss = m.loss_and_grad(x.to(DEV), y.to(DEV), noise=noise.to(DEV))
    grads = {k: p.grad.cpu().numpy().copy() for k, p in m.named_parameters()}
    m.adam_step(1)
    with default_f64():
        o = getattr(oest, 'Oracle' + cls)(eps_noise=float(g['eps_noise']), **extra, **kw)
        o.load_state_dict(_w0(g))
        if cls == 'MDRFF':
            _double_oracle_rff(o)
        opt = torch.optim.Adam(o.parameters(), lr=kw['lr'])
        ref_loss = o.mdn_loss_fn(*o.forward(x.double(), noise=noise.double()), y.double())
        ref_loss.backward()
        ref_grads = {k: p.grad.numpy().copy() for k, p in o.named_parameters()}
        opt.step()
    assert abs(float(loss.item()) - float(ref_loss.item())) <= 1e-12 * abs(float(ref_loss.item()))
    assert float(loss.item()) == pytest.approx(float(g['loss']), rel=1e-5)
    for k in grads:
        _close(grads[k], ref_grads[k], 1e-12, 'grad ' + k)
        scale = max(np.abs(g['grad.' + k]).max(), 1e-8)          # the fp32 test's tolerances
        np.testing.assert_allclose(grads[k], g['grad.' + k], rtol=1e-3, atol=2e-5 * scale, err_msg=k)
    lr = float(g['lr'])
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float64
        _close(v.cpu().numpy(), o.state_dict()[k].numpy(), 1e-12, 'w1 ' + k)
    # Adam in isolation, as the fp32 test does it: the golden gradients in, the golden weights out
    m.load_state_dict(_w0(g))
    m._exp_avg.zero_(), m._exp_avg_sq.zero_()
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.grad.copy_(torch.from_numpy(g['grad.' + k]))
    m.adam_step(1)
    for k, v in m.state_dict().items():
        # the fp32 test's tolerance on the golden fp32 weights, which are fp32 numbers: the fp64 result is
        # compared as .float() gives it
        np.testing.assert_allclose(v.float().cpu().numpy(), g['w1.' + k], rtol=0, atol=1e-4 * lr, err_msg=k)


DEEP_TRUNKS = [((16, 12, 8), act, False) for act in ('Tanh', 'ReLU', 'LeakyReLU', 'Sigmoid', 'Identity')] + \
    [((16, 12, 8), 'Tanh', True), ((12,) * 8, 'Tanh', False), ((12,) * 8, 'ReLU', False)]


@pytest.mark.parametrize('hidden,act,full', DEEP_TRUNKS, ids=lambda v: str(v).replace(' ', ''))
def test_one_step_grads_on_deeper_trunks(B, hidden, act, full):
    """The per-phase pass away from the reference's defaults: trunks of three and of eight (the maximum)
    layers, every activation, both covariance shapes.  fp32-representable weights and data, a given noise;
    loss and every parameter's gradient within 1e-12 of the fp64 oracle, the rule of the one-step test above
    (the oracle's own spread over four orders of the input columns at these shapes: <= 6.7e-16)."""
    from oracle import estimators as oest
    d, k, b, i = 3, 3, 32, 10
    B.MDNN.EPS_NOISE = 1e-5
    kw = dict(input_dim=i, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d), n_gaussians=k,
              full_covariance=full, hidden_layers=hidden, activation=getattr(torch.nn, act), lr=1e-3)
    torch.manual_seed(11)
    m = B.MDNN(device=DEV, **kw)
    w0 = {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
    m.double()
    gen = torch.Generator().manual_seed(12)
    x, y, noise = torch.randn(b, i, generator=gen), torch.rand(b, d, generator=gen), torch.rand(b, d, k, generator=gen)
    loss = m.loss_and_grad(x.to(DEV), y.to(DEV), noise=noise.to(DEV))
    grads = {n: p.grad.cpu().numpy().copy() for n, p in m.named_parameters()}
    with default_f64():
        o = oest.OracleMDNN(eps_noise=1e-5, **kw)
        o.load_state_dict(w0)
        ref_loss = o.mdn_loss_fn(*o.forward(x.double(), noise=noise.double()), y.double())
        ref_loss.backward()
        ref_grads = {n: p.grad.numpy().copy() for n, p in o.named_parameters()}
    assert len(grads) == 2 * (len(hidden) + (4 if full else 3)) and set(grads) == set(ref_grads)
    _close(float(loss.item()), float(ref_loss.item()), 1e-12, 'loss')
    for n in grads:
        _close(grads[n], ref_grads[n], 1e-12, 'grad ' + n)


# ------------------------------------------------------------------ chunks
CHUNKS = {
    'mdnn_start': dict(cls='MDNN', summarizer='summary_start', d=2, k=10, hidden=(24, 24), full=False),
    'mdnn_corrdiff_full': dict(cls='MDNN', summarizer='summary_corrdiff', d=3, k=3, hidden=(16, 16), full=True),
    'mdrff_corrdiff': dict(cls='MDRFF', summarizer='summary_corrdiff', d=4, k=4, hidden=[], full=False),
}
N_ORDERS = 8
# updates of each chunk that are compared (the condition on the oracle's own spread, below, decides)
N_UPDATES = {'mdnn_start': 100, 'mdnn_corrdiff_full': 100, 'mdrff_corrdiff': 100}


def _chunk_kw(tag, g, input_dim):
    kw = CHUNKS[tag]
    d = kw['d']
    common = dict(input_dim=input_dim, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d),
                  n_gaussians=kw['k'], full_covariance=kw['full'], lr=float(g['lr']), activation=torch.nn.Tanh)
    if kw['cls'] == 'MDRFF':
        common.update(n_feat=200, sigma=4.0, kernel='RBF', freqs=g['rff.freqs'])
    else:
        common.update(hidden_layers=kw['hidden'])
    return common


def _result(logs, weights, fwd):
    out = {'train_loss': np.asarray(logs['train_loss'], np.float64),
           'test_loss': np.asarray(logs['test_loss'], np.float64)}
    out.update({'w.' + k: np.asarray(v, np.float64) for k, v in weights.items()})
    for name, v in zip(('mog.w', 'mog.mu', 'mog.l_d', 'mog.low'), fwd):
        if v is not None:
            out[name] = np.asarray(v, np.float64)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_orders(tag):
    """_oracle_orders_on the chunk's reference-made summaries and ids.  Run once, shared."""
    g = golden('chunk_%s.npz' % tag)
    return _oracle_orders_on(tag, torch.from_numpy(g['summaries']).double(), g['ids'][:N_UPDATES[tag]])


def _oracle_orders_on(tag, s64, ids):
    """The fp64 oracle on the chunk as it is (order 0) and with the input columns -- and the first layer's
    weight columns (an MDRFF: the frequencies' and sigma's) with them -- permuted, as tests/test_gpu_fit.py
    builds its evaluation orders."""
    from oracle import estimators as oest
    g = golden('chunk_%s.npz' % tag)
    kw, nu = CHUNKS[tag], len(ids)
    theta = torch.from_numpy(g['theta']).double()
    n_train = int(s64.shape[0] * 0.8)
    w0 = _w0(g)
    runs = []
    with default_f64():
        for i in range(N_ORDERS):
            perm = None if i == 0 else torch.from_numpy(np.random.RandomState(100 + i).permutation(s64.shape[1]))
            ckw = _chunk_kw(tag, g, s64.shape[1])
            w = {k: v.clone() for k, v in w0.items()}
            x = s64
            if perm is not None:
                x = s64[:, perm].contiguous()
                if kw['cls'] == 'MDRFF':
                    ckw['freqs'] = g['rff.freqs'][:, perm.numpy()]
                else:
                    w['net.fcon0.weight'] = w0['net.fcon0.weight'][:, perm].contiguous()
            o = getattr(oest, 'Oracle' + kw['cls'])(eps_noise=0.0, **ckw)
            o.load_state_dict(w)
            if kw['cls'] == 'MDRFF':
                _double_oracle_rff(o)
            logs = o.run_training(x, theta, nu, int(g['batch']), ids_table=ids)
            sd = {k: v.detach().numpy().copy() for k, v in o.state_dict().items()}
            if perm is not None and kw['cls'] == 'MDNN':
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(perm.numel())
                sd['net.fcon0.weight'] = sd['net.fcon0.weight'][:, inv.numpy()]
            with torch.no_grad():
                fwd = [None if t is None else t.numpy().copy() for t in o.forward(x[n_train:n_train + 1])]
            runs.append(_result(logs, sd, fwd))
    return runs


@functools.lru_cache(maxsize=None)
def _device_chunk(tag, dtype):
    import bayes_sim_ig_amd as B
    g = golden('chunk_%s.npz' % tag)
    nu = N_UPDATES[tag]
    old, B.MDNN.EPS_NOISE = B.MDNN.EPS_NOISE, 0.0
    try:
        summ = torch.from_numpy(g['summaries']).to(DEV)
        theta = torch.from_numpy(g['theta']).to(DEV)
        kw = _chunk_kw(tag, g, summ.shape[1])
        m = getattr(B, CHUNKS[tag]['cls'])(device=DEV, **kw)
        m.load_state_dict(_w0(g))
        if dtype == 'float64':
            m.double()
        logs = m.run_training(summ, theta, nu, int(g['batch']), ids_table=g['ids'][:nu])
        n_train = int(summ.shape[0] * 0.8)
        fwd = [None if t is None else t.cpu().numpy() for t in m.forward(summ[n_train:n_train + 1])]
        mog = m.predict_MoGs(summ[n_train:n_train + 1])[0]
        sd = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    finally:
        B.MDNN.EPS_NOISE = old
    return _result(logs, sd, fwd), mog, m


def _assert_rule6(hip, runs, what):
    """|hip - ref| <= 8 max_i |order_i - ref| + 1e-11 |ref|, given that the oracle's own spread over the
    orders is <= 1e-8 relative at every logging point."""
    ref = runs[0]
    report = []
    for key in ('train_loss', 'test_loss'):
        spread = np.max([np.abs(r[key] - ref[key]) for r in runs[1:]], axis=0)
        rel = (spread / np.abs(ref[key])).max()
        report.append('%s %s: oracle spread %.3g' % (what, key, rel))
        assert rel <= 1e-8, 'condition broken: shorten the chunk (%s %s: %.3g)' % (what, key, rel)
    for key in ref:
        spread = np.max([np.abs(r[key] - ref[key]) for r in runs[1:]], axis=0)
        dev = np.abs(hip[key] - ref[key])
        bound = 8 * spread + 1e-11 * np.abs(ref[key])
        scale = max(np.abs(ref[key]).max(), 1e-300)
        report.append('%s %s: spread %.3g, HIP deviation %.3g (of max |ref|)' %
                      (what, key, spread.max() / scale, dev.max() / scale))
        print(report[-1])
        assert (dev <= bound).all(), (report[-1], float((dev - bound).max()))
    return report


@pytest.mark.parametrize('tag', list(CHUNKS))
def test_teacher_forced_chunk_matches_fp64_oracle(B, tag):
    hip, mog, _ = _device_chunk(tag, 'float64')
    runs = _oracle_orders(tag)
    assert len(hip['train_loss']) == 6 and len(hip['test_loss']) == 6
    _assert_rule6(hip, runs, tag)
    # predict_MoGs: the forward tuple above, de-normalised on the unit box (lows 0, highs 1: unchanged)
    assert mog.a.dtype == np.float64
    np.testing.assert_array_equal(mog.a, hip['mog.w'][0])
    np.testing.assert_array_equal(np.stack([c.m for c in mog.xs]), hip['mog.mu'][0].T)
    d = CHUNKS[tag]['d']
    rows, cols = np.tril_indices(d, -1)
    for k, c in enumerate(mog.xs):
        t = np.diag(hip['mog.l_d'][0][:, k])
        if 'mog.low' in hip:
            t[rows, cols] = hip['mog.low'][0][:, k]
        np.testing.assert_allclose(c.S, t @ t.T, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('tag', list(CHUNKS))
def test_fp64_logs_agree_with_the_fp32_device_path(B, tag):
    f64, _, _ = _device_chunk(tag, 'float64')
    f32, _, _ = _device_chunk(tag, 'float32')
    for key in ('train_loss', 'test_loss'):
        np.testing.assert_allclose(f32[key], f64[key], rtol=1e-4, atol=1e-5, err_msg=key)


# ------------------------------------------------------------------ BayesSim
def _diag_cov(l_d):
    """[K, D, D] covariances of a diagonal forward tuple's l_d [1, D, K]"""
    return np.stack([np.diag(l_d[0][:, k] ** 2) for k in range(l_d.shape[2])])


@pytest.mark.parametrize('tag', ['mdrff_corrdiff', 'mdnn_start'])
def test_bayessim_float64(B, tag):
    """fit + predict on one trajectory through BayesSim({... 'dtype': 'float64'}) on the chunk's 250 pairs
    (mdrff_corrdiff: Cartpole-shaped, I = 302) against the fp64 oracle under rule 6: the oracle runs, in
    eight orders, on the device-made summaries widened to double, with the minibatch ids the same numpy seed
    gives."""
    g = golden('chunk_%s.npz' % tag)
    kw = CHUNKS[tag]
    B.MDNN.EPS_NOISE = 0.0
    states, actions = torch.from_numpy(g['states']).to(DEV), torch.from_numpy(g['actions']).to(DEV)
    theta = torch.from_numpy(g['theta']).to(DEV)
    nu, batch = int(g['n_updates']), int(g['batch'])
    cfg = {'modelClass': kw['cls'], 'summarizerFxn': kw['summarizer'], 'trainTrajLen': states.shape[1],
           'components': kw['k'], 'hiddenLayers': kw['hidden'], 'lr': float(g['lr']), 'dtype': 'float64'}
    np.random.seed(0)
    bs = B.BayesSim(model_cfg=cfg, obs_dim=states.shape[2], act_dim=actions.shape[2], params_dim=kw['d'],
                    params_lows=np.zeros(kw['d']), params_highs=np.ones(kw['d']), prior=None, device=DEV)
    assert bs.model._f64 and bs.model.input_dim == g['summaries'].shape[1]
    if kw['cls'] == 'MDRFF':
        bs.model.rff.freqs = torch.from_numpy(g['rff.freqs']).float().to(DEV)
        bs.model._bufs.pop('coeff64', None)
    bs.model.load_state_dict(_w0(g))
    old = (B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE)
    B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = nu, batch
    try:
        np.random.seed(77)
        logs = bs.fit(theta, states, actions)
    finally:
        B.BayesSim.NUM_GRAD_UPDATES, B.BayesSim.MINIBATCH_SIZE = old
    assert len(logs) == 1 and len(logs[0]['test_loss']) == 6
    n_train = int(states.shape[0] * 0.8)
    mog = bs.predict(states[n_train:n_train + 1], actions[n_train:n_train + 1])
    assert mog.a.dtype == np.float64
    got = {'train_loss': np.asarray(logs[0]['train_loss']), 'test_loss': np.asarray(logs[0]['test_loss']),
           'mog.w': mog.a[None], 'mog.mu': np.stack([c.m for c in mog.xs]).T[None],
           'mog.S': np.stack([c.S for c in mog.xs])}
    # the oracle's side: the summaries the device made (fp32, widened), the ids of the same numpy draw
    np.random.seed(77)
    ids = np.random.randint(0, n_train, (nu, batch), dtype=np.int32)
    s64 = bs._summarize(states, actions).cpu().double()
    runs = []
    for r in _oracle_orders_on(tag, s64, ids):
        runs.append({'train_loss': r['train_loss'], 'test_loss': r['test_loss'], 'mog.w': r['mog.w'],
                     'mog.mu': r['mog.mu'], 'mog.S': _diag_cov(r['mog.l_d'])})
    _assert_rule6(got, runs, 'BayesSim ' + tag)


def test_bayessim_float64_refit_matches_oracle(B):
    """predict on several trajectories with a double model: the refit (bayes_sim.py:148-179; full covariance,
    input_dim = 1, a (128, 128) trunk) in float64 -- tests/test_gpu_fit.py's
    test_bayessim_multi_trajectory_refit_matches_oracle with a float64 model and the oracle under default
    dtype float64, at that test's 1e-4 for 2000 samples (same samples, same torch-RNG start weights, same
    numpy ids)."""
    from oracle import estimators as oest
    g = golden('pendulum_ref.npz')
    B.MDNN.EPS_NOISE = 0.0
    n, n_samples, tol = g['params'].shape[0], 2000, 1e-4
    sa = torch.from_numpy(g['data']).reshape(n, -1, 4).to(DEV)
    cfg = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_start', 'trainTrajLen': 10, 'components': 3,
           'hiddenLayers': (128, 128), 'lr': 5e-4, 'fullCovariance': True, 'dtype': 'float64'}
    torch.manual_seed(3)
    bsim = B.BayesSim(model_cfg=cfg, obs_dim=3, act_dim=1, params_dim=2, params_lows=np.array([0.01] * 2),
                      params_highs=np.array([2.0] * 2), prior=None, proposal=None, device=DEV)
    np.random.seed(9)
    bsim.run_training(torch.from_numpy(g['params']).to(DEV), sa[:, :, :3].contiguous(), sa[:, :, 3:].contiguous())
    tsa = sa[[5, 17, 40]]
    st, ac = tsa[:, :, :3].contiguous(), tsa[:, :, 3:].contiguous()
    old, B.BayesSim.REFIT_SAMPLES = B.BayesSim.REFIT_SAMPLES, n_samples
    try:
        np.random.seed(31)
        torch.manual_seed(32)
        mog = bsim.predict(st, ac)
        # the same flow, the refit by the oracle: built under the default dtype the device model's CPU
        # initialisation runs under (same torch-RNG draws), then widened like the device model
        np.random.seed(31)
        torch.manual_seed(32)
        mogs = bsim.model.predict_MoGs(bsim._summarize(st, ac))
        o = oest.OracleMDNN(input_dim=1, output_dim=2, output_lows=np.array([0.01] * 2),
                            output_highs=np.array([2.0] * 2), n_gaussians=3, full_covariance=True,
                            hidden_layers=(128, 128), activation=torch.nn.Tanh, lr=5e-4, eps_noise=0.0).double()
        # (the box bounds are plain attributes: widened fp32 values, as the device model holds them)
        o.output_lows, o.output_highs = o.output_lows.double(), o.output_highs.double()
        smpls = torch.from_numpy(np.concatenate([m.gen(n_samples=n_samples // 3) for m in mogs], axis=0)).double()
        with default_f64():
            inp = torch.zeros(smpls.shape[0], 1)
            o.run_training(inp, smpls, B.BayesSim.REFIT_EPOCHS * n_samples // 100, 100)
            w, ms, ls = o.predict_mog_params(inp[0:1])[0]
    finally:
        B.BayesSim.REFIT_SAMPLES = old
    assert mog.ndim == 2 and mog.a.dtype == np.float64 and mog.xs[0].m.dtype == np.float64
    ref = B.pdf.MoG(a=w, ms=ms, Ls=ls)
    np.testing.assert_allclose(mog.a, ref.a, rtol=tol, atol=tol * 1e-2)
    got_m, ref_m = np.stack([c.m for c in mog.xs]), np.stack([c.m for c in ref.xs])
    got_s, ref_s = np.stack([c.S for c in mog.xs]), np.stack([c.S for c in ref.xs])
    print('refit: max |a - ref| %.3g, max |m - ref| %.3g' % (np.abs(mog.a - ref.a).max(), np.abs(got_m - ref_m).max()))
    np.testing.assert_allclose(got_m, ref_m, rtol=tol, atol=tol * 1e-1)
    scale = np.abs(ref_s).max(axis=(1, 2), keepdims=True)
    assert (np.abs(got_s - ref_s) <= tol * scale + 1e-9).all(), (got_s - ref_s) / scale
    th = np.array([[1.0, 0.5]])
    np.testing.assert_allclose(mog.eval(th, log=True), ref.eval(th, log=True), rtol=tol, atol=tol)


# ------------------------------------------------------------------ determinism and flags
def test_two_fp64_fits_are_bitwise_equal_and_float_goes_back(B):
    tag = 'mdnn_corrdiff_full'
    a, _, m = _device_chunk(tag, 'float64')
    _device_chunk.cache_clear()
    b, _, _ = _device_chunk(tag, 'float64')
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    # .float() after a double fit: the fp32 run_training still works on the model
    g = golden('chunk_%s.npz' % tag)
    B.MDNN.EPS_NOISE = 0.0
    m.float()
    assert m._flat.dtype == torch.float32
    logs = m.run_training(torch.from_numpy(g['summaries']).to(DEV), torch.from_numpy(g['theta']).to(DEV),
                          20, int(g['batch']), ids_table=g['ids'][:20])
    assert np.isfinite(logs['test_loss']).all() and logs['test_loss'][-1] < a['test_loss'][0]


def test_nan_in_theta_raises_like_the_fp32_path(B):
    g = golden('chunk_mdnn_start.npz')
    B.MDNN.EPS_NOISE = 0.0
    summ = torch.from_numpy(g['summaries']).to(DEV)
    theta = torch.from_numpy(g['theta']).clone()
    theta[3, 0] = float('nan')
    m = B.MDNN(device=DEV, **_chunk_kw('mdnn_start', g, summ.shape[1]))
    m.load_state_dict(_w0(g))
    m.double()
    ids = np.tile(np.arange(10), (5, 1))      # every minibatch holds row 3
    with pytest.raises(AssertionError):
        m.run_training(summ, theta.to(DEV), 5, 10, ids_table=ids)


def test_c_abi_refuses_what_the_fp64_mode_does_not_cover(B):
    L = B._lib
    lib = L.load()
    g = golden('chunk_mdnn_start.npz')
    m = B.MDNN(device=DEV, **_chunk_kw('mdnn_start', g, 40)).double()
    cfg = m._cfg()
    plan = C.c_void_p()
    L.check(lib.bsig_fit64_create(C.byref(cfg), C.byref(m._hyper()), 10, 80, 20, 5, C.byref(plan)))
    try:
        fb = L.Fit64Buffers()
        assert lib.bsig_fit64_bind(plan, C.byref(fb), L.FIT_SPLIT_ADAM) == L.BSIG_EUNSUPPORTED
        assert b'data-parallel' in lib.bsig_last_error()
        fb.x_kind = L.X_CROSSCORR_FACTORS
        assert lib.bsig_fit64_bind(plan, C.byref(fb), 0) == L.BSIG_EUNSUPPORTED
        assert b'factor rows' in lib.bsig_last_error()
    finally:
        lib.bsig_fit64_destroy(plan)
