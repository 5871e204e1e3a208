"""Every device path of the mixture-density head (csrc/mdn_head.hip, the row code of
csrc/head_device.h) element by element against the fp64 oracle
(oracle.estimators.mdn_head_closed_form).

The case table (tests/head_cases.py) reaches the one-wavefront-per-row kernel with its 2-, 4- and
8-sweep row bodies, the thread-per-component diagonal and full-covariance kernels, partial last
workgroups, and the multi-slab finishing kernel; every case first checks its path through
bsig_debug_head_geometry.  Tolerances are those of test_gpu_kernels.py's
test_head_nll_and_grad_match_closed_form unless a comment says otherwise.

A jitter scale of EPS_NOISE = 1e-5 moves sigma by 1e-5 of its mean: too little for a wrong draw or
a wrong jitter-scale gradient term to show at these tolerances.  The cases marked `eps` therefore
also run at eps_noise = 0.25, where both are O(1e-1) of the result."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_cases as H
from oracle import estimators as oest

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS_BIG = 0.25
SEED, STREAM = 0x5EED1234ABCD, 77
IDS = [H.case_id(c) for c in H.CASES]


@pytest.fixture(scope='module')
def B():
    import bayes_sim_ig_amd as pkg
    pkg._lib.require_gpu()
    pkg.MDNN.VERBOSE = False
    return pkg


def _dims(B, d, k, full, eps, min_w=oest.MIN_WEIGHT, ll=oest.LL_LIMIT):
    hd = B._lib.HeadDims()
    hd.out_dim, hd.n_comp, hd.full_cov = d, k, 1 if full else 0
    hd.eps_noise, hd.min_weight, hd.ll_limit = eps, min_w, ll
    return hd


def _check_geometry(B, case):
    batch, d, k, full, path, body, multi = case
    out = (C.c_int32 * 16)()
    assert B._lib.load().bsig_debug_head_geometry(C.byref(_dims(B, d, k, full, 0.0)), batch, out) == 0
    assert (out[0], out[1], out[6] > 1) == (path, body, multi), list(out)
    return list(out)


def _data(case, seed=0):
    """raw head outputs (fp32, some logits large enough for the MIN_WEIGHT clamp), targets, noise"""
    batch, d, k, full = case[:4]
    nh = k + 2 * d * k + (d * (d - 1) // 2 if full else 0) * k
    gen = torch.Generator().manual_seed(batch * 7 + d * 131 + k + seed)
    o = torch.randn(batch, nh, generator=gen) * 0.5
    o[:, :k] *= 6.0
    y = torch.rand(batch, d, generator=gen)
    noise = torch.rand(batch, d, k, generator=gen)
    return o.numpy(), y.numpy(), noise.numpy()


def _ws(B, hd, batch):
    n = int(B._lib.load().bsig_head_workspace_bytes(C.byref(hd), batch))
    assert n > 0
    return torch.empty(n // 4 + 64, device=DEV)


def _head_nll(B, hd, o, ld, y, ldy, batch, noise=None, rows=None, norm_batch=None, seed=0, sid=0,
              d_out=None):
    """bsig_mdn_head_nll on device tensors; returns (loss, d_out, nonfinite flag)"""
    lib = B._lib.load()
    loss = torch.full((1,), float('nan'), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    if d_out is None:
        d_out = torch.full((batch, ld), float('nan'), device=DEV)
    ws = _ws(B, hd, batch)
    B._lib.check(lib.bsig_mdn_head_nll(
        C.byref(hd), B._lib.ptr(o), ld, B._lib.ptr(y), ldy, B._lib.ptr(rows), batch,
        norm_batch or batch, B._lib.ptr(noise), seed, sid, B._lib.ptr(loss), B._lib.ptr(d_out),
        B._lib.ptr(flag), B._lib.ptr(ws), ws.numel() * 4, B._lib.stream()))
    torch.cuda.synchronize()
    return float(loss.item()), d_out, int(flag.item())


def _loss_tol(geo, batch, ref, lse):
    """the existing head test's bound (2e-6 relative / absolute), and for a batch of more than 1024
    rows the fp32 summation of the row logsumexps on top: each row's value passes through at most R
    adds inside its workgroup, ceil(blocks / 1024) per thread and a 6-level wavefront tree plus 16
    wavefront partials in the finishing kernel, each add off by at most 2^-24 of the running sum"""
    tol = 2e-6 * max(1.0, abs(ref))
    if batch > 1024:
        depth = geo[2] + -(-geo[5] // 1024) + 6 + 16
        tol += depth * 2.0**-24 * np.abs(lse).mean()
    return tol


def _assert_head(loss, d_out, ref_loss, ref_grad, aux, geo, batch, nh, msg=''):
    assert abs(loss - ref_loss) <= _loss_tol(geo, batch, ref_loss, aux['lse']), (loss, ref_loss, msg)
    gscale = np.abs(ref_grad).max()
    np.testing.assert_allclose(d_out[:, :nh], ref_grad, rtol=2e-4, atol=2e-6 * gscale, err_msg=msg)


# ------------------------------------------------------------------ NLL + gradient, injected noise
@pytest.mark.parametrize('eps', [0.0, 1e-5, EPS_BIG])
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_nll_and_grad_vs_fp64(B, case, eps):
    geo = _check_geometry(B, case)
    batch, d, k, full = case[:4]
    o, y, noise = _data(case)
    nh = o.shape[1]
    ref, ref_g, aux = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=eps, noise=noise)
    loss, d_o, flag = _head_nll(B, _dims(B, d, k, full, eps), torch.from_numpy(o).to(DEV), nh,
                                torch.from_numpy(y).to(DEV), d, batch,
                                noise=torch.from_numpy(noise).to(DEV))
    assert flag == 0
    _assert_head(loss, d_o.cpu().numpy(), ref, ref_g, aux, geo, batch, nh)


# ------------------------------------------------------------------ drawn noise (Philox on the device)
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_drawn_noise_vs_fp64(B, case):
    """noise = NULL: the kernel draws u itself.  The oracle regenerates u with the path's element ->
    draw mapping (head_cases.draws_wave / draws_flat): every (row, d, k) has its own draw in every
    row body, the lanes past groups * K and the rows of a partial workgroup included."""
    geo = _check_geometry(B, case)
    batch, d, k, full, path = case[:5]
    o, y, _ = _data(case, seed=1)
    nh = o.shape[1]
    u = H.draws_for_path(path, batch, d, k, SEED, STREAM)
    ref, ref_g, aux = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=EPS_BIG, noise=u)
    loss, d_o, flag = _head_nll(B, _dims(B, d, k, full, EPS_BIG), torch.from_numpy(o).to(DEV), nh,
                                torch.from_numpy(y).to(DEV), d, batch, seed=SEED, sid=STREAM)
    assert flag == 0
    _assert_head(loss, d_o.cpu().numpy(), ref, ref_g, aux, geo, batch, nh)


# ------------------------------------------------------------------ gathered targets, norm_batch
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_gathered_targets_and_norm_batch(B, case):
    """y_rows into a larger target pool whose unreferenced rows are NaN, norm_batch = 3 * batch:
    the loss is the plain one, every gradient (the jitter-scale term too) scales by batch / norm_batch."""
    geo = _check_geometry(B, case)
    batch, d, k, full = case[:4]
    o, y, noise = _data(case, seed=2)
    nh = o.shape[1]
    rng = np.random.RandomState(batch + d)
    pool = 2 * batch + 3
    rows = rng.randint(0, pool, batch).astype(np.int32)
    y_pool = np.full((pool, d), np.nan, np.float32)
    y_pool[rows] = y
    ref, ref_g, aux = oest.mdn_head_closed_form(o, y_pool[rows], d, k, full, eps_noise=EPS_BIG,
                                                noise=noise)
    loss, d_o, flag = _head_nll(B, _dims(B, d, k, full, EPS_BIG), torch.from_numpy(o).to(DEV), nh,
                                torch.from_numpy(y_pool).to(DEV), d, batch,
                                noise=torch.from_numpy(noise).to(DEV),
                                rows=torch.from_numpy(rows).to(DEV), norm_batch=3 * batch)
    assert flag == 0
    _assert_head(loss, d_o.cpu().numpy(), ref, ref_g * (batch / (3 * batch)), aux, geo, batch, nh)


# ------------------------------------------------------------------ padded pitch
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_padded_pitch(B, case):
    """ld = Nh + 5 with NaN in the padding of head_out: the padding is never read (the loss and
    gradients stay finite and right) and d_head_out's padding keeps its contents."""
    geo = _check_geometry(B, case)
    batch, d, k, full = case[:4]
    o, y, noise = _data(case, seed=3)
    nh = o.shape[1]
    ld = nh + 5
    o_pad = np.full((batch, ld), np.nan, np.float32)
    o_pad[:, :nh] = o
    ref, ref_g, aux = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=EPS_BIG, noise=noise)
    d_out = torch.full((batch, ld), 1234.5, device=DEV)
    loss, d_o, flag = _head_nll(B, _dims(B, d, k, full, EPS_BIG), torch.from_numpy(o_pad).to(DEV),
                                ld, torch.from_numpy(y).to(DEV), d, batch,
                                noise=torch.from_numpy(noise).to(DEV), d_out=d_out)
    assert flag == 0
    d_o = d_o.cpu().numpy()
    assert (d_o[:, nh:] == 1234.5).all()
    _assert_head(loss, d_o, ref, ref_g, aux, geo, batch, nh)


# ------------------------------------------------------------------ clamps
def _threshold_in_gap(values, lo_q, hi_q):
    """the middle of the widest gap between the sorted values in the [lo_q, hi_q] quantile range
    (no value sits near it: fp32 and fp64 agree on which side every value is), and the gap"""
    v = np.sort(np.asarray(values).ravel())
    if v.size == 1:                 # (one value: half of it, the value clamped)
        return 0.5 * v[0], 0.5 * v[0]
    a, b = int(lo_q * (v.size - 1)), max(int(hi_q * (v.size - 1)), int(lo_q * (v.size - 1)) + 1)
    v = v[a:b + 1]
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1]), v[i + 1] - v[i]


@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_clamps_vs_fp64(B, case):
    """A tiny ll_limit (about half the components' logp clamped, their gradients masked) and a large
    min_weight (clamped softmax outputs, renormalised weights under the second clamp), both placed in
    the widest gap of the data, against the oracle with the same settings.  In a tall batch a few
    values still sit within fp32 rounding of a threshold, where fp32 and fp64 may take different
    sides of a mask: the gradients a mask there gates are left out (the loss is continuous across)."""
    geo = _check_geometry(B, case)
    batch, d, k, full = case[:4]
    o, y, noise = _data(case, seed=4)
    nh = o.shape[1]
    aux0 = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=1e-5, noise=noise)[2]
    ll = _threshold_in_gap(np.abs(aux0['logp']), 0.3, 0.7)[0]
    s = np.exp(o[:, :k].astype(np.float64) - o[:, :k].max(axis=1, keepdims=True))
    s /= s.sum(axis=1, keepdims=True)
    min_w = 0.5 if k == 1 else _threshold_in_gap(s, 0.2, 0.6)[0]
    ref, ref_g, aux = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=1e-5, noise=noise,
                                                min_weight=min_w, ll_limit=ll)
    clamped = np.abs(aux['logp']) > ll
    assert clamped.any() and (clamped.size == 1 or (~clamped).any())
    if k > 1:
        assert (s < min_w).any() and (aux['weights'] < min_w).any()
    loss, d_o, flag = _head_nll(B, _dims(B, d, k, full, 1e-5, min_w, ll), torch.from_numpy(o).to(DEV),
                                nh, torch.from_numpy(y).to(DEV), d, batch,
                                noise=torch.from_numpy(noise).to(DEV))
    assert flag == 0
    # (fp32 logp: a few ulp of its terms; softmax / renormalised weights: about K ulp)
    near_lp = np.abs(np.abs(aux['logp']) - ll) <= 2e-5 * ll                        # [B, K]
    near_w = ((np.abs(s - min_w) <= 1e-5 * min_w) |
              (np.abs(aux['weights'] - min_w) <= 1e-5 * min_w)).any(axis=1)        # [B]
    keep = np.ones((batch, nh), bool)
    keep[near_w, :k] = False
    ls = d * (d - 1) // 2 if full else 0
    for blk, n in ((k, d), (k + d * k, d), (k + 2 * d * k, ls)):
        keep[:, blk:blk + n * k] &= ~np.tile(near_lp, (1, n))
    assert keep.mean() > 0.99
    d_o = d_o.cpu().numpy()
    _assert_head(loss, np.where(keep, d_o[:, :nh], ref_g), ref, ref_g, aux, geo, batch, nh)


# ------------------------------------------------------------------ forward() tuple, tuple loss
@pytest.mark.parametrize('drawn', [False, True])
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_outputs_and_tuple_loss_vs_fp64(B, case, drawn):
    """bsig_mdn_head_outputs (weights, mu, L_d, lower) against the oracle's tuple, with injected and
    with drawn noise (flat element mapping); bsig_mdn_nll_from_tuple of the fp64 tuple rounded to
    fp32 against the fp64 loss of that rounded tuple."""
    geo = _check_geometry(B, case)
    batch, d, k, full = case[:4]
    ls = d * (d - 1) // 2 if full else 0
    o, y, noise = _data(case, seed=5)
    lib = B._lib.load()
    if drawn:
        noise = H.draws_flat(batch, d, k, SEED, STREAM)
    aux = oest.mdn_head_closed_form(o, y, d, k, full, eps_noise=EPS_BIG, noise=noise)[2]
    hd = _dims(B, d, k, full, EPS_BIG)
    w = torch.full((batch, k), float('nan'), device=DEV)
    mu = torch.full((batch, d * k), float('nan'), device=DEV)
    l_d = torch.full((batch, d * k), float('nan'), device=DEV)
    low = torch.full((batch, max(ls * k, 1)), float('nan'), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = _ws(B, hd, batch)
    nz = None if drawn else torch.from_numpy(noise.astype(np.float32)).to(DEV)
    B._lib.check(lib.bsig_mdn_head_outputs(
        C.byref(hd), B._lib.ptr(torch.from_numpy(o).to(DEV)), o.shape[1], batch, B._lib.ptr(nz),
        SEED, STREAM, B._lib.ptr(w), B._lib.ptr(mu), B._lib.ptr(l_d),
        B._lib.ptr(low) if full else None, B._lib.ptr(flag), B._lib.ptr(ws), ws.numel() * 4,
        B._lib.stream()))
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    # softmax of K fp32 terms, clamp, renormalisation: a few ulp per term summed
    np.testing.assert_allclose(w.cpu().numpy(), aux['weights'], rtol=2e-5, atol=0)
    np.testing.assert_array_equal(mu.cpu().numpy(), aux['mu'].reshape(batch, -1).astype(np.float32))
    np.testing.assert_allclose(l_d.cpu().numpy(), aux['l_d'].reshape(batch, -1), rtol=5e-6, atol=0)
    if full:
        np.testing.assert_array_equal(low.cpu().numpy(),
                                      aux['lower'].reshape(batch, -1).astype(np.float32))
    # the loss of the rounded fp64 tuple
    t32 = [aux['weights'].astype(np.float32), aux['mu'].astype(np.float32),
           aux['l_d'].astype(np.float32), aux['lower'].astype(np.float32) if full else None]
    ref = oest.mdn_nll_from_tuple(*t32, y, full)
    dev = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) if t is not None else None for t in t32]
    loss = torch.full((1,), float('nan'), device=DEV)
    yd = torch.from_numpy(y).to(DEV)
    ws = _ws(B, hd, batch)
    B._lib.check(lib.bsig_mdn_nll_from_tuple(
        C.byref(hd), *[B._lib.ptr(t) for t in dev], B._lib.ptr(yd), d, batch, B._lib.ptr(loss),
        B._lib.ptr(flag), B._lib.ptr(ws), ws.numel() * 4, B._lib.stream()))
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert abs(float(loss.item()) - ref) <= _loss_tol(geo, batch, ref, aux['lse'])


# ------------------------------------------------------------------ non-finite flag
@pytest.mark.parametrize('case', H.CASES, ids=IDS)
def test_head_nonfinite_flag_from_last_row(B, case):
    """A NaN in the last mean of the last row (the last workgroup, the last sweep) raises the flag,
    in the NLL kernel and in the forward() tuple kernel.  The NLL stays finite (the logp clamp's
    fmin / fmax drop the NaN), so the flag there is the row's own check, not the finishing kernel's."""
    _check_geometry(B, case)
    batch, d, k, full = case[:4]
    o, y, noise = _data(case, seed=6)
    nh = o.shape[1]
    o[batch - 1, k + d * k - 1] = np.nan
    hd = _dims(B, d, k, full, 1e-5)
    od = torch.from_numpy(o).to(DEV)
    loss, _, flag = _head_nll(B, hd, od, nh, torch.from_numpy(y).to(DEV), d, batch,
                              noise=torch.from_numpy(noise).to(DEV))
    assert flag == 1 and np.isfinite(loss)
    ls = d * (d - 1) // 2 if full else 0
    outs = [torch.empty(batch, n, device=DEV) for n in (k, d * k, d * k, max(ls * k, 1))]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = _ws(B, hd, batch)
    B._lib.check(B._lib.load().bsig_mdn_head_outputs(
        C.byref(hd), B._lib.ptr(od), nh, batch, B._lib.ptr(torch.from_numpy(noise).to(DEV)), 0, 0,
        *[B._lib.ptr(t) for t in outs], B._lib.ptr(flag), B._lib.ptr(ws), ws.numel() * 4,
        B._lib.stream()))
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


# ------------------------------------------------------------------ refused shape
def test_head_refused_shape_writes_nothing(B):
    """Full covariance at D48 K10 needs more than 64 KB of LDS for one row: the launch is refused
    with an error naming LDS, and neither the loss nor d_head_out is written."""
    batch, d, k, full = H.REFUSED
    lib = B._lib.load()
    hd = _dims(B, d, k, full, 1e-5)
    nh = int(lib.bsig_head_width(C.byref(hd)))
    out = (C.c_int32 * 16)()
    assert lib.bsig_debug_head_geometry(C.byref(hd), batch, out) == B._lib.BSIG_EUNSUPPORTED
    o = torch.randn(batch, nh, device=DEV)
    y = torch.rand(batch, d, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    d_o = torch.full((batch, nh), 3.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)
    rc = lib.bsig_mdn_head_nll(C.byref(hd), B._lib.ptr(o), nh, B._lib.ptr(y), d, None, batch, batch,
                               None, 0, 0, B._lib.ptr(loss), B._lib.ptr(d_o), B._lib.ptr(flag),
                               B._lib.ptr(ws), ws.numel() * 4, B._lib.stream())
    assert rc == B._lib.BSIG_EUNSUPPORTED
    assert 'LDS' in lib.bsig_last_error().decode()
    torch.cuda.synchronize()
    assert float(loss.item()) == 7.0 and bool((d_o == 3.0).all()) and int(flag.item()) == 0


# ------------------------------------------------------------------ MDNN.loss_and_grad, tall batches
@pytest.mark.parametrize('batch', [1025, 8193])
@pytest.mark.parametrize('d', [13, 32])
def test_loss_and_grad_tall_batch_vs_fp64_autograd(B, batch, d):
    """MDNN.loss_and_grad at minibatches past 1024 rows (head bias column sums over several finish
    slabs; exp-sum partials delivered by the head GEMM) against fp64 autograd of OracleMDNN, with
    the tolerances of test_one_step_grads_and_adam_match_reference."""
    k, inp = 10, 40
    kw = dict(input_dim=inp, output_dim=d, n_gaussians=k, full_covariance=False,
              hidden_layers=(64, 64), lr=1e-3, output_lows=np.zeros(d), output_highs=np.ones(d),
              activation=torch.nn.Tanh)
    old = B.MDNN.EPS_NOISE
    B.MDNN.EPS_NOISE = 1e-5
    try:
        torch.manual_seed(batch + d)
        m = B.MDNN(device=DEV, **kw)
        gen = torch.Generator().manual_seed(batch * 3 + d)
        x = torch.randn(batch, inp, generator=gen)
        y = torch.rand(batch, d, generator=gen)
        noise = torch.rand(batch, d, k, generator=gen)
        loss = m.loss_and_grad(x.to(DEV), y.to(DEV), noise=noise.to(DEV))
        torch.cuda.synchronize()
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)    # the oracle's fp32 `result` buffer in fp64 too
        try:
            ref = oest.OracleMDNN(eps_noise=1e-5, **kw).double()
            ref.load_state_dict({n: v.detach().cpu().double() for n, v in m.state_dict().items()})
            ref_loss = ref.mdn_loss_fn(*ref.forward(x.double(), noise=noise.double()), y.double())
            ref_loss.backward()
        finally:
            torch.set_default_dtype(prev)
        assert float(loss.item()) == pytest.approx(float(ref_loss.item()), rel=1e-5)
        grads = dict(ref.named_parameters())
        for name, p in m.named_parameters():
            r = grads[name].grad.numpy()
            scale = max(np.abs(r).max(), 1e-8)
            np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=1e-3, atol=2e-5 * scale,
                                       err_msg=name)
    finally:
        B.MDNN.EPS_NOISE = old
