"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol
include/bsig.h declares, the Python mirror keeps the reference's interface
(state_dict keys, torch-RNG init order, numpy-RNG frequency draw, error
behaviour) and the product path refuses to run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import head_cases as H
import summary_cases as S

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib, pdf
from oracle import estimators as oest

NO_GPU = not torch.cuda.is_available()


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, 'bayes_sim_ig_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert 'oracle' not in src.replace('Oracle of record', ''), fn


def test_summary_dim_matches_reference_shapes():
    g = golden('summaries.npz')
    for case in ('cartpole', 'ant', 'short', 'pendulum'):
        s, a = g[case + '.states'], g[case + '.actions']
        for fn in ('summary_start', 'summary_corr', 'summary_corrdiff'):
            if case + '.' + fn in g:
                assert B.summarizers.summary_dim(fn, s.shape[1], s.shape[2], a.shape[2]) \
                    == g[case + '.' + fn].shape[1]
    for d, depth in zip(g['signature_depth.d'], g['signature_depth.depth']):
        assert B.signature_depth(int(d)) == int(depth)
    assert B.summarizers.summary_dim('summary_signatory', 11, 211, 20) == 232
    assert B.summarizers.summary_dim('summary_signatory', 11, 17, 4) == 22 + 22 ** 2 + 22 ** 3


@pytest.mark.parametrize('full', [False, True])
def test_mdnn_matches_reference_interface(full):
    kw = dict(input_dim=40, output_dim=3, output_lows=np.zeros(3), output_highs=np.ones(3),
              n_gaussians=10, full_covariance=full, hidden_layers=(24, 24),
              activation=torch.nn.Tanh, lr=5e-4)
    torch.manual_seed(3)
    m = B.MDNN(device='cpu', **kw)
    torch.manual_seed(3)
    o = oest.OracleMDNN(**kw)
    assert list(m.state_dict()) == list(o.state_dict())
    for a, b in zip(m.state_dict().values(), o.state_dict().values()):
        assert torch.equal(a, b)                   # same torch-RNG init order
    assert m.L_size == 3 and m.n_gaussians == 10 and m.lr == 5e-4
    assert isinstance(m, torch.nn.Module) and m.activation is torch.nn.Tanh
    # parameters are views of one flat buffer; load_state_dict writes through
    sd = {k: torch.full_like(v, 0.25) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    used = sum(p.numel() for p in m.parameters())
    assert float(m._flat.sum()) == pytest.approx(0.25 * used)
    assert m._flat.numel() % 4 == 0
    assert all(p.grad is not None and p.grad.data_ptr() >= m._flat_grad.data_ptr()
               for p in m.parameters())


def test_mdrff_frequency_draw_consumes_numpy_rng_like_reference():
    np.random.seed(11)
    m = B.MDRFF(input_dim=302, output_dim=13, output_lows=np.zeros(13),
                output_highs=np.ones(13), n_gaussians=4, lr=1e-3, activation=torch.nn.Tanh,
                full_covariance=False, n_feat=64, sigma=4.0)
    np.random.seed(11)
    ref = np.random.normal(0.0, 1.0, (32, 302))
    np.testing.assert_array_equal(m.rff.freqs.numpy(), ref.astype(np.float32))
    assert m.rff.a == pytest.approx(np.sqrt(2.0 / 64))
    assert list(m.state_dict()) == ['pi.weight', 'pi.bias', 'mu.weight', 'mu.bias',
                                    'Diag.0.weight', 'Diag.0.bias']
    assert m.pi.weight.shape == (4, 64)
    with pytest.raises(ValueError):
        B.RFF(64, 302, 4.0, kernel='Bogus', quasi_random=False)


@pytest.mark.parametrize('tag', ['cos_rbf'] + ['%s.%s' % (k, m)
                                               for k in ('Matern12', 'Matern32', 'Matern52',
                                                         'Laplace')
                                               for m in ('cossin', 'cos')])
def test_rff_variant_draws_are_the_references(tag):
    """f4 (host half): the product RFF consumes the numpy RNG like the reference's RFF for the
    cos-only map (freqs, then 2*pi*rand offsets, rff.py:98-102) and for the Matern / Laplace
    Student-t draws (normal, then chisquare, rff.py:151-184): frequencies, offsets and the RNG
    state afterwards equal the reference-generated golden bit for bit."""
    g = golden('rff_variants.npz')
    if tag == 'cos_rbf':
        args = dict(n_feat=64, d=302, sigma=4.0, cos_only=True, kernel='RBF')
    else:
        kern, mode = tag.split('.')
        args = dict(n_feat=48, d=150, sigma=[0.5 + 0.01 * j for j in range(150)],
                    cos_only=(mode == 'cos'), kernel=kern)
    np.random.seed(int(g[tag + '.seed']))
    r = B.RFF(quasi_random=False, device='cpu', **args)
    assert int(np.random.randint(0, 1 << 30)) == int(g[tag + '.rng_after'])
    np.testing.assert_array_equal(r.freqs.numpy(), g[tag + '.freqs'])
    assert float(r.a) == float(g[tag + '.a'])
    if args['cos_only']:
        np.testing.assert_array_equal(r.offset.numpy(), g[tag + '.offset'])
    else:
        assert r.offset is None


@pytest.mark.skipif(not NO_GPU, reason='checks the no-GPU failure mode')
def test_product_path_fails_loudly_without_gpu():
    m = B.MDNN(input_dim=4, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2),
               n_gaussians=2, full_covariance=False, hidden_layers=(8,),
               activation=torch.nn.Tanh, lr=1e-3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.forward(torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.run_training(torch.zeros(10, 4), torch.zeros(10, 2), 2, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        B.summary_start(torch.zeros(1, 12, 3), torch.zeros(1, 12, 1))


def test_bayessim_constructs_by_name_like_reference():
    cfg = {'modelClass': 'MDRFF_Matern52_2.5', 'summarizerFxn': 'summary_corrdiff',
           'trainTrajLen': 21, 'components': 4, 'hiddenLayers': (128, 128), 'lr': 1e-3}
    B.MDNN.VERBOSE = False
    np.random.seed(0)
    bs = B.BayesSim(model_cfg=cfg, obs_dim=4, act_dim=1, params_dim=13,
                    params_lows=np.zeros(13), params_highs=np.ones(13), prior=None)
    assert isinstance(bs.model, B.MDRFF) and bs.model.rff.n_feat == 200
    assert bs.model.input_dim == 302 and float(bs.model.rff.sigma[0, 0]) == 2.5
    assert B.BayesSim.NUM_GRAD_UPDATES == 100 and B.BayesSim.MINIBATCH_SIZE == 100
    assert B.BayesSim.get_n_trajs_per_batch(2500, 2000) == 500
    with pytest.raises(NameError):
        B.BayesSim(model_cfg=dict(cfg, summarizerFxn='nope'), obs_dim=4, act_dim=1,
                   params_dim=13, params_lows=np.zeros(13), params_highs=np.ones(13),
                   prior=None)


def test_bayessim_matern_model_by_name_draws_the_references_model():
    """f4: BayesSim(modelClass='MDRFF_Matern32_2.0') under the seeds make_golden.chunk_case used
    builds the reference's model: same torch-RNG head init, same numpy-RNG Student-t frequencies
    (bayes_sim.py:72-81, rff.py:167-170), sigma 2.0."""
    g = golden('chunk_mdrff_matern32.npz')
    cfg = {'modelClass': 'MDRFF_Matern32_2.0', 'summarizerFxn': 'summary_corrdiff',
           'trainTrajLen': 21, 'components': 4, 'hiddenLayers': [], 'lr': 1e-3,
           'fullCovariance': False}
    B.MDNN.VERBOSE = False
    torch.manual_seed(24)
    np.random.seed(24)
    bs = B.BayesSim(model_cfg=cfg, obs_dim=4, act_dim=1, params_dim=4,
                    params_lows=np.zeros(4), params_highs=np.ones(4), prior=None)
    np.testing.assert_array_equal(bs.model.rff.freqs.numpy(), g['rff.freqs'])
    np.testing.assert_array_equal(bs.model.rff.sigma.numpy(), g['rff.sigma'])
    for k, v in bs.model.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g['w0.' + k])


def test_compat_aliases():
    from bayes_sim_ig_amd import compat
    compat.install()
    from bayes_sim_ig.bayes_sim import BayesSim
    from bayes_sim_ig.models.mdnn import MDNN
    from bayes_sim_ig.models.mdrff import MDRFF
    from bayes_sim_ig.utils.summarizers import summary_corrdiff
    from bayes_sim_ig.utils import pdf as p2
    assert BayesSim is B.BayesSim and MDNN is B.MDNN and MDRFF is B.MDRFF
    assert summary_corrdiff is B.summary_corrdiff and p2 is pdf


def test_pdf_matches_reference():
    g = golden('pdf_cases.npz')
    for tag in ('full', 'diag'):
        mog = pdf.MoG(a=g['a'], ms=list(g['ms']), Ls=list(g['Ls_' + tag]))
        np.testing.assert_allclose(mog.eval(g['x'], log=True), g['logpdf_' + tag], rtol=1e-12)
        np.testing.assert_allclose(mog.eval(g['x'], log=False), g['pdf_' + tag], rtol=1e-12)
        np.testing.assert_allclose(np.stack([c.S for c in mog.xs]), g['S_' + tag], rtol=1e-12)
        np.testing.assert_allclose(np.stack([c.P for c in mog.xs]), g['P_' + tag], rtol=1e-9)
        np.testing.assert_allclose([c.logdetP for c in mog.xs], g['logdetP_' + tag], rtol=1e-12)
        np.random.seed(77)
        np.testing.assert_allclose(mog.gen(n_samples=50), g['gen_' + tag], rtol=1e-12)
    mog = pdf.MoG(a=np.array([0.6, 0.001, 0.397, 0.002]), ms=list(g['ms']),
                  Ls=list(g['Ls_full']))
    mog.prune_negligible_components(threshold=0.005)
    np.testing.assert_allclose(mog.a, g['pruned_a'], rtol=1e-14)
    np.testing.assert_allclose(np.stack([c.m for c in mog.xs]), g['pruned_ms'])
    uni = pdf.Uniform(np.zeros(3), np.ones(3) * 2.0)
    np.testing.assert_allclose(uni.eval(g['uniform_x']), g['uniform_logpdf'])
    np.random.seed(78)
    np.testing.assert_allclose(uni.gen(n_samples=5), g['uniform_gen'])
    # product / quotient round trip (py3 __truediv__)
    prior = pdf.Gaussian(m=np.zeros(3), S=4.0 * np.eye(3))
    back = (mog * prior) / prior
    np.testing.assert_allclose(back.a, mog.a, rtol=1e-9)
    np.testing.assert_allclose(back.xs[0].m, mog.xs[0].m, rtol=1e-8, atol=1e-10)


def test_quasi_random_frequencies_are_not_collinear():
    """RFF with input_dim <= 100 draws its frequencies from a low-discrepancy sequence
    (reference rff.py:113-117 via mdrff.py:23).  A PLAIN Halton sequence would make every
    coordinate with a prime base above m the same ramp (for m = 100, I = 40: 14 collinear,
    one-sided columns); the stand-in for ghalton's generalized sequence must not."""
    import numpy as np
    from bayes_sim_ig_amd import rff
    m, d = 100, 40                          # BayesSim's default nFeat = 200 on pendulum summary_start
    pts = rff.halton_points(m, d)
    assert pts.shape == (m, d) and pts.min() > 0.0 and pts.max() < 1.0
    assert np.array_equal(pts, rff.halton_points(m, d))          # deterministic
    f = rff.draw_freqs('RBF', m, d, quasi_random=True)
    c = np.corrcoef(f.T)
    np.fill_diagonal(c, 0.0)
    assert np.abs(c).max() < 0.5                                 # iid normal columns: ~0.3
    assert np.abs(f.mean(0)).max() < 0.3 and 0.8 < f.std(0).min() and f.std(0).max() < 1.2
    # low discrepancy survives the scrambling: every coordinate fills its 10 deciles evenly
    counts = np.stack([np.histogram(pts[:, j], bins=10, range=(0, 1))[0] for j in range(d)])
    assert counts.min() >= 5 and counts.max() <= 15           # iid uniform: 2..20


def test_narrow_two_layer_trunk_is_stored_zero_padded():
    """A two-layer tanh trunk narrower than 128 lives zero-padded to [128, 128] in the flat
    buffer (so that the persistent update kernel covers it); the module surface -- parameter
    shapes, state_dict keys, load_state_dict -- is the reference's."""
    import numpy as np
    import torch
    from bayes_sim_ig_amd import MDNN
    kw = dict(input_dim=40, output_dim=2, output_lows=np.zeros(2), output_highs=np.ones(2),
              n_gaussians=10, full_covariance=True, activation=torch.nn.Tanh, lr=1e-3)
    torch.manual_seed(3)
    m = MDNN(hidden_layers=(24, 24), **kw)
    torch.manual_seed(3)
    ref = MDNN(hidden_layers=(128, 128), **kw)
    assert m._hidden == [24, 24] and m._hidden_stored == [128, 128]
    assert m._flat.numel() == ref._flat.numel()
    sd = m.state_dict()
    assert list(sd) == list(ref.state_dict())
    assert sd['net.fcon0.weight'].shape == (24, 40) and sd['net.fcon1.weight'].shape == (24, 24)
    assert sd['pi.weight'].shape == (10, 24) and sd['Lower.weight'].shape == (10, 24)
    total_real = sum(v.numel() for v in sd.values())
    assert int((m._flat != 0).sum()) <= total_real
    # the same torch-RNG stream as an unpadded (24, 24) reference-shaped model
    torch.manual_seed(3)
    lin = torch.nn.Linear(40, 24)
    assert torch.equal(sd['net.fcon0.weight'], lin.weight.detach())
    # load_state_dict writes through the views into the flat buffer
    new = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    m.load_state_dict(new)
    assert float(m._flat.sum()) == 0.5 * total_real
    m.net[0].weight.grad.fill_(1.0)
    assert float(m._flat_grad.sum()) == 24 * 40
    # three layers, relu, wide trunks: stored as they are
    assert MDNN(hidden_layers=(24, 24, 24), **kw)._hidden_stored == [24, 24, 24]
    assert MDNN(hidden_layers=(24, 24), **dict(kw, activation=torch.nn.ReLU))._hidden_stored == [24, 24]
    assert MDNN(hidden_layers=(256, 64), **kw)._hidden_stored == [256, 64]


def test_linear_head_tiling_planner():
    """The tiling of the persistent kernel of the linear heads (csrc/fit_persistent.hip, host
    arithmetic: bsig_debug_persist_geometry): the ShadowHand head gets 32 x 192 tiles on 198 CUs and
    two rows per owner on 50 of the CUs to spare; every covered shape respects the chip (<= 256
    workgroups, <= 160 KB of LDS each), owns every minibatch row and every held-out row."""
    import ctypes as C
    import numpy as np
    lib = _lib.load()
    names = ['NT', 'KS', 'n_blocks', 'k_slices', 'G', 'T', 'n_owner', 'R', 'NE', 'RE', 'eval_passes', 'lds', 'mixed']

    def geom(batch, feat, d, k, max_test):
        out = (C.c_int32 * 16)()
        ok = lib.bsig_debug_persist_geometry(batch, feat, d, k, max_test, out)
        return ok, dict(zip(names, list(out)[:13]))

    ok, g = geom(100, 4096, 32, 4, 200)          # cfg5: 260 x 4096 heads
    assert ok and (g['NT'], g['KS'], g['n_blocks'], g['k_slices']) == (2, 192, 9, 22)
    assert (g['G'], g['T'], g['n_owner'], g['R'], g['mixed']) == (198, 248, 50, 2, 0)
    ok, g = geom(100, 1024, 13, 10, 200)         # cfg2: 270 x 1024
    assert ok and g['NT'] == 1 and g['KS'] == 96 and g['mixed'] == 0
    rng = np.random.RandomState(0)
    n_ok = 0
    for _ in range(300):
        batch, k = int(rng.randint(1, 113)), int(rng.randint(1, 17))
        d = int(rng.randint(1, min(40, 8 * (64 // k)) + 1))
        feat = int(rng.choice([96, 200, 300, 500, 512, 1024, 2048, 4096, 8192]))
        max_test = int(rng.randint(0, 400))
        ok, g = geom(batch, feat, d, k, max_test)
        if not ok:
            continue
        n_ok += 1
        nh = k * (1 + 2 * d)
        assert g['KS'] in (96, 192, 288) and g['NT'] in (1, 2)
        assert g['n_blocks'] * 16 * g['NT'] >= nh and g['k_slices'] * g['KS'] >= feat
        assert g['G'] == g['n_blocks'] * g['k_slices'] <= 256 and g['G'] <= g['T'] <= 256
        assert g['n_owner'] * g['R'] >= batch and 1 <= g['R'] <= 8 and g['n_owner'] <= g['T']
        assert g['lds'] <= 160 * 1024
        if g['eval_passes'] > 0:
            assert g['NE'] * g['RE'] >= max_test and g['RE'] <= 8 and g['NE'] <= g['T']
            assert g['eval_passes'] * batch >= max_test
        # owners on workgroups of their own unless the chip has none to spare
        assert g['mixed'] == max(0, g['n_owner'] - (g['T'] - g['G']))
    assert n_ok > 200
    assert geom(200, 4096, 32, 4, 0)[0] == 0        # minibatches beyond 112 rows: the v1 kernel / per-phase kernels


def test_mdnn_kernel_workgroup_planner():
    """The layout of the persistent kernel of the two-layer MDNN (csrc/fit_persistent_mdnn.hip, host
    arithmetic: bsig_debug_persist_mdnn_geometry): an owner workgroup takes ONE minibatch row where the
    chip has the CUs for a workgroup per row (narrow first layers), else two, else four; first layers with
    more tiles than CUs are streamed (8 rows per owner); every covered shape respects the chip."""
    import ctypes as C
    import numpy as np
    lib = _lib.load()
    names = ['k_slices', 'G1', 'n_owner', 'mr', 'n_small', 'wide', 'stream', 'eval_passes', 'lds', 'Nh']

    def geom(batch, inp, d, k, full=0, max_test=200):
        out = (C.c_int32 * 16)()
        ok = lib.bsig_debug_persist_mdnn_geometry(batch, inp, d, k, full, max_test, out)
        return ok, dict(zip(names, list(out)[:10]))

    ok, g = geom(100, 232, 32, 4)                 # cfg4: one k-slice, a workgroup per row
    assert ok and (g['k_slices'], g['G1'], g['mr'], g['n_owner'], g['wide'], g['stream']) == (1, 4, 1, 100, 0, 0)
    ok, g = geom(100, 11802, 10, 5)               # cfg3-like: 47 k-slices, two rows per owner
    assert ok and (g['k_slices'], g['G1'], g['mr'], g['n_owner'], g['stream']) == (47, 188, 2, 50, 0)
    ok, g = geom(100, 11802, 17, 10)              # cfg/ant.yaml: wide heads
    assert ok and g['wide'] == 1 and g['mr'] == 2 and g['G1'] + g['n_owner'] + g['n_small'] <= 256
    ok, g = geom(100, 56402, 13, 10)              # cfg/anymal.yaml: streamed first layer
    assert ok and g['stream'] == 1 and g['mr'] == 8 and g['n_owner'] == 13
    ok, g = geom(100, 232, 4, 4, full=1)          # full covariance keeps four rows per owner
    assert ok and g['mr'] == 4 and g['n_owner'] == 25
    rng = np.random.RandomState(1)
    n_ok = 0
    for _ in range(300):
        batch, k = int(rng.randint(1, 105)), int(rng.randint(1, 17))
        d = int(rng.randint(1, min(40, 8 * (64 // k)) + 1))
        inp = int(rng.choice([3, 40, 190, 256, 257, 1290, 2310, 11154, 11802, 12300, 13000, 56402]))
        ok, g = geom(batch, inp, d, k, 0, int(rng.randint(0, 400)))
        if not ok:
            continue
        n_ok += 1
        assert g['Nh'] == k * (1 + 2 * d) and g['k_slices'] * 256 >= inp
        assert g['G1'] + g['n_owner'] + g['n_small'] <= 256 and g['lds'] <= 160 * 1024
        assert g['n_owner'] * g['mr'] >= batch and g['mr'] in (1, 2, 4, 8)
        if not g['stream']:
            assert g['G1'] == 4 * g['k_slices']
            # the fewest rows per owner the chip has CUs for
            for mr in (1, 2):
                if mr < g['mr']:
                    assert 4 * g['k_slices'] + -(-batch // mr) + g['n_small'] > 256
        else:
            assert g['mr'] == 8 and inp % 2 == 0
    assert n_ok > 150


# ------------------------------------------------ mixture-density head paths (host arithmetic)
HEAD_GEOM = ['path', 'body', 'R', 'threads', 'lds', 'blocks', 'slabs', 'rows_per_slab', 'nq', 'Nh']


def head_geometry(batch, d, k, full):
    """bsig_debug_head_geometry: (return code, dict of its outputs)"""
    import ctypes as C
    hd = _lib.HeadDims()
    hd.out_dim, hd.n_comp, hd.full_cov = d, k, 1 if full else 0
    hd.eps_noise, hd.min_weight, hd.ll_limit = 1e-5, 1e-5, 1e5
    out = (C.c_int32 * 16)(*([-1] * 16))
    rc = _lib.load().bsig_debug_head_geometry(C.byref(hd), batch, out)
    assert list(out)[len(HEAD_GEOM):] == [0] * (16 - len(HEAD_GEOM))
    return rc, dict(zip(HEAD_GEOM, list(out)))


def test_philox_known_answers():
    """tests/head_cases.py's Philox4x32-10 (the mirror of common.h the drawn-noise GPU tests
    regenerate the jitter from): the Random123 known answers."""
    got = H.philox4x32_10(0, 0, np.zeros(1, np.uint64))[0]
    assert ['%08x' % v for v in got] == ['6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']
    got = H.philox4x32_10(2**64 - 1, 2**64 - 1, np.array([2**64 - 1], np.uint64))[0]
    assert ['%08x' % v for v in got] == ['408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd']


def test_jitter_draw_mappings():
    """The two element -> draw mappings of head_cases: every (row, d, k) of a row gets its own
    Philox word (the wavefront mapping uses all four words of a counter and two counters per lane),
    and the rows do not share draws."""
    for b, d, k in [(3, 48, 10), (2, 8, 64), (2, 40, 3), (2, 1, 1)]:
        for fn in (H.draws_wave, H.draws_flat):
            u = fn(b, d, k, 7, 11)
            assert u.shape == (b, d, k) and (u >= 0).all() and (u < 1).all()
            assert len(np.unique(u)) == u.size            # 24-bit draws: no collision at these sizes
    # element (d = 7, k = 2) of row 1 at K = 10: lane 1 * 10 + 2 of sweep 1, counter (64 + 12) * 2, word 1
    u = H.draws_wave(2, 13, 10, 5, 9)
    w = H.philox4x32_10(5, 9, np.array([(64 + 12) * 2], np.uint64))[0]
    assert u[1, 7, 2] == (int(w[1]) >> 8) / 2.0**24
    u = H.draws_flat(2, 13, 10, 5, 9)
    w = H.philox4x32_10(5, 9, np.array([(13 + 7) * 10 + 2], np.uint64))[0]
    assert u[1, 7, 2] == (int(w[0]) >> 8) / 2.0**24


@pytest.mark.parametrize('case', H.CASES, ids=[H.case_id(c) for c in H.CASES])
def test_head_case_table_resolves_to_its_path(case):
    batch, d, k, full, path, body, multi = case
    rc, g = head_geometry(batch, d, k, full)
    assert rc == 0
    assert (g['path'], g['body'], g['slabs'] > 1) == (path, body, multi)
    assert g['Nh'] == k + 2 * d * k + (d * (d - 1) // 2 if full else 0) * k
    assert g['nq'] == -(-d // (64 // k)) and g['lds'] <= 64 * 1024
    assert g['blocks'] == -(-batch // g['R']) and g['threads'] % 64 == 0
    assert g['slabs'] * g['rows_per_slab'] >= batch and g['slabs'] <= 64
    if path in (0, 1):
        assert (g['R'], g['threads']) == (8, 512)
    else:
        assert g['threads'] >= g['R'] * k


def test_head_case_table_covers_every_path():
    """The GPU head tests' case table reaches every device path and row body, tall batches, partial
    blocks, and the component counts where lane arithmetic goes wrong."""
    got = {(c[4], c[5]) for c in H.CASES}
    assert got >= {(H.PATH_WAVE2, 2), (H.PATH_WAVE8, 4), (H.PATH_WAVE8, 8), (H.PATH_DIAG, 0),
                   (H.PATH_FULL, 0)}
    assert {1, 7, 1001, 1025, 8193} <= {c[0] for c in H.CASES}
    assert {1, 3, 7, 10, 16, 33, 64} <= {c[2] for c in H.CASES}
    for path in (H.PATH_WAVE2, H.PATH_WAVE8, H.PATH_DIAG, H.PATH_FULL):
        assert any(c[6] for c in H.CASES if c[4] == path), H.PATH_NAMES[path]   # multi-slab finish
    # partial last workgroups: 7 rows of an 8-row wavefront block, 1001 rows of an R-row block
    for c in H.CASES:
        if c[0] in (7, 1001):
            g = head_geometry(*c[:4])[1]
            assert c[0] % g['R'] != 0 or g['R'] == 1, H.case_id(c)
    assert 1001 % head_geometry(1001, 49, 10, False)[1]['R'] == 1


@pytest.mark.parametrize('k', [1, 3, 7, 10, 16, 33, 64])
def test_head_path_boundaries_in_d(k):
    """Two sweeps -> the 4-sweep body at D = 2 * (64 / K) + 1, -> the 8-sweep body at 4 * (64 / K) + 1,
    -> the thread-per-component kernel at nine sweeps."""
    g = 64 // k
    for d, want in [(2 * g, (0, 2)), (2 * g + 1, (1, 4)), (4 * g, (1, 4)), (4 * g + 1, (1, 8)),
                    (8 * g, (1, 8)), (8 * g + 1, (2, 0))]:
        rc, geo = head_geometry(100, d, k, False)
        assert rc == 0 and (geo['path'], geo['body']) == want, (d, k, geo)
        assert geo['nq'] == -(-d // g)


def test_head_finish_slab_boundaries():
    for batch, slabs, rows in [(1024, 1, 1024), (1025, 9, 114), (8192, 64, 128), (8193, 64, 129)]:
        for shape in [(13, 10, False), (49, 10, False), (4, 16, True)]:
            rc, g = head_geometry(batch, *shape)
            assert rc == 0 and (g['slabs'], g['rows_per_slab']) == (slabs, rows), (batch, shape, g)


def test_head_full_covariance_lds_limit():
    """Full covariance: D32 K10 fits one row per workgroup; D48 K10 needs more than 64 KB and is
    refused with the error a launch returns."""
    for batch in (1, 1025, 8193):
        rc, g = head_geometry(batch, 32, 10, True)
        assert rc == 0 and (g['path'], g['R'], g['threads']) == (3, 1, 64)
    rc, g = head_geometry(*H.REFUSED)
    assert rc == _lib.BSIG_EUNSUPPORTED and all(v == 0 for v in g.values())
    assert 'LDS' in _lib.load().bsig_last_error().decode()
    # ... as a launch of it does, before it touches the device
    hd = _lib.HeadDims()
    hd.out_dim, hd.n_comp, hd.full_cov = 48, 10, 1
    assert _lib.load().bsig_head_workspace_bytes(ctypes.byref(hd), 4) == 0


# ------------------------------------------------ summarizer paths (host arithmetic)
def summary_path(*args):
    """bsig_debug_summary_path: (return code, dict of its outputs)"""
    out = (ctypes.c_int32 * 16)(*([-1] * 16))
    rc = _lib.load().bsig_debug_summary_path(*args, out)
    assert list(out)[len(S.PATH_FIELDS):] == [0] * (16 - len(S.PATH_FIELDS))
    return rc, dict(zip(S.PATH_FIELDS, list(out)))


@pytest.mark.parametrize('case', S.CASES, ids=[S.case_id(c) for c in S.CASES])
def test_summary_case_table_resolves_to_its_path(case):
    rc, p = summary_path(*S.query_args(case))
    assert rc == 0, _lib.load().bsig_last_error()
    assert (p['kernel'], p['store'], p['prefetch']) == (case.kernel, case.store, case.prefetch), p
    for k, v in case.want.items():
        assert p[k] == v, (k, p)
    n = case.n
    if case.kernel == S.K_WAVE:
        s, a = S.dims(case)
        assert (p['threads'], p['lds'], p['grid']) == (256, 16 * (s + a), min(-(-n // 4), 65536))
    else:
        assert p['grid'] == min(n, S.GRID_CAP) and p['threads'] % 64 == 0
    if case.kind in (S.CORR, S.CORRDIFF):
        s, a = S.dims(case)
        assert p['steps'] == S.window(case.t, case.sd)
        assert (p['ex_x'], p['ex_y']) == (min(-(-(s * a + 2) // 256), 64), min(n, S.GRID_CAP))
        if case.kernel != S.K_WAVE:
            assert p['threads'] == 256 and p['lds'] == 4 * (s + a + 8)
        assert (p['rstep'] > 0) == (case.store == S.ST_QUAD)
        if case.kernel == S.K_QUADS:     # 128-byte runs: rstep A/4 quads a multiple of 8
            assert p['rstep'] * (a // 4) % 8 == 0 and p['rstep'] * (a // 4) <= 256
    elif case.kind == S.SIG:
        d = 1 + case.sd + case.ad
        assert p['depth'] == S.sig_depth(case) and p['steps'] == case.t
        if case.kernel == S.K_SIG3:
            assert p['threads'] == -(-d * d // 64) * 64 and p['dmax'] >= d > p['dmax'] - 8
            assert p['prefetch'] == (case.t * case.sd <= p['threads'] and case.t * case.ad <= p['threads'])
    else:
        assert p['steps'] == case.max_t


def test_summary_case_table_covers_every_path():
    """The GPU summarizer tests' case table reaches every kernel, store loop and fetch, the
    boundaries between them, and a second trajectory per workgroup on each grid-striding path."""
    got = {(c.kernel, c.store, c.prefetch) for c in S.CASES}
    assert got >= {(S.K_START, S.ST_ELEM, 0), (S.K_WAVE, S.ST_ELEM, 0), (S.K_WAVE, S.ST_FACTORS, 0),
                   (S.K_QUADS, S.ST_QUAD, 1)} | \
        {(S.K_CC, st, pf) for st in (S.ST_QUAD, S.ST_VEC4_TAIL, S.ST_FACTORS) for pf in (0, 1)} | \
        {(S.K_CC, st, 1) for st in (S.ST_VEC4, S.ST_ELEM)} | \
        {(S.K_SIG3, st, 1) for st in (S.ST_LINE, S.ST_ELEM)} | \
        {(S.K_SIG3, S.ST_LINE, 0), (S.K_SIG12, S.ST_ELEM, 0)}
    assert {8, 16, 24, 32} <= {c.want.get('dmax') for c in S.CASES}
    assert {c.want['threads'] for c in S.CASES if c.kind == S.START} == {64, 128, 256}
    assert {1, 2} <= {S.sig_depth(c) for c in S.CASES if c.kernel == S.K_SIG12}
    assert {1, 8, 24, 128, 256} <= {c.want.get('rstep') for c in S.CASES if c.kernel == S.K_QUADS}
    assert any(c.max_t != 10 for c in S.CASES if c.kind == S.START)
    assert any(c.t != c.ta for c in S.CASES if c.kind == S.START)
    big = {(c.kernel, c.store, c.prefetch) for c in S.CASES if c.n > S.GRID_CAP}
    assert big >= {(c.kernel, c.store, c.prefetch) for c in S.CASES
                   if c.kernel in (S.K_QUADS, S.K_CC, S.K_SIG3)}
    assert any(c.n >= S.N_WAVE for c in S.CASES if c.kernel == S.K_WAVE and not c.factors)
    assert any(c.n >= S.N_WAVE for c in S.CASES if c.kernel == S.K_WAVE and c.factors)
    # the wide factor rows whose expansion grid-strides in x (S A + 2 > 64 x 256), and in y
    assert any(c.factors and S.dims(c)[0] * S.dims(c)[1] + 2 > 64 * 256 for c in S.CASES)
    assert any(c.factors and c.n > S.GRID_CAP for c in S.CASES)


def _cc_case(t, sd, ad, n=5, **kw):
    return S.C('x', S.CORRDIFF, n, t, t, sd, ad, 0, 0, 0, **kw)


@pytest.mark.parametrize('shape,want', [
    ((4, 129, 1), S.K_WAVE), ((4, 130, 1), S.K_QUADS),          # S A = 2048 | 2064
    ((8, 33, 1), S.K_WAVE), ((8, 34, 1), S.K_QUADS),            # S A = 2048 | 2112
    ((6, 257, 4), S.K_QUADS), ((6, 258, 4), S.K_CC),            # sd - 1 = 256 | 257
    ((3, 3, 256), S.K_QUADS), ((3, 3, 257), S.K_CC),            # ad = 256 | 257
    ((3, 3, 300), S.K_CC), ((11, 300, 2), S.K_CC)])
def test_crosscorr_path_boundaries(shape, want):
    c = _cc_case(*shape)
    rc, p = summary_path(*S.query_args(c))
    assert rc == 0 and p['kernel'] == want, (shape, p)
    s, a = S.dims(c)
    if want == S.K_WAVE:
        assert s * a == 2048
    else:
        assert s * a > 2048 and p['prefetch'] == (c.sd - 1 <= 256 and c.ad <= 256)
    # factor rows never take the quads kernel; a misaligned or odd pitch drops the float4 stores
    rc, p = summary_path(*S.query_args(c._replace(factors=True)))
    assert rc == 0 and p['kernel'] == (S.K_WAVE if want == S.K_WAVE else S.K_CC)
    assert p['store'] == S.ST_FACTORS
    for odd in (c._replace(off=1), c._replace(pad=1 if (S.width(c) + 1) % 4 else 2)):
        rc, p = summary_path(*S.query_args(odd))
        assert rc == 0 and (p['kernel'], p['store']) == \
            ((S.K_WAVE, S.ST_ELEM) if want == S.K_WAVE else (S.K_CC, S.ST_ELEM)), (odd, p)


def test_crosscorr_quads_rstep_boundaries():
    """rstep = (256 / (A/4)) rounded down to a multiple of 8 / gcd(A/4, 8): 1 at A/4 = 136, 0 (the
    workgroup kernel's quad store, 256 / (A/4) rows per sweep) at A/4 = 35 and 150."""
    for shape, kernel, rstep in [((8, 3, 68), S.K_QUADS, 1), ((21, 8, 14), S.K_CC, 7),
                                 ((21, 3, 60), S.K_CC, 1), ((4, 130, 1), S.K_QUADS, 256),
                                 ((51, 60, 8), S.K_QUADS, 24), ((21, 48, 12), S.K_QUADS, 8)]:
        rc, p = summary_path(*S.query_args(_cc_case(*shape)))
        assert rc == 0 and (p['kernel'], p['store'], p['rstep']) == (kernel, S.ST_QUAD, rstep), shape


def test_crosscorr_generic_store_boundaries():
    # A % 4 != 0: generic float4 loop; its scalar tail exactly when S A % 4 != 0
    for shape, store in [((21, 25, 1), S.ST_VEC4), ((5, 52, 3), S.ST_VEC4_TAIL),
                         ((21, 20, 110), S.ST_VEC4), ((21, 20, 102), S.ST_QUAD),   # A = 1100 | 1020
                         ((3, 3, 257), S.ST_VEC4_TAIL)]:
        c = _cc_case(*shape)
        rc, p = summary_path(*S.query_args(c))
        s, a = S.dims(c)
        assert rc == 0 and (p['kernel'], p['store']) == (S.K_CC, store), (shape, p)
        assert (store == S.ST_VEC4_TAIL) == ((s * a) % 4 != 0)


@pytest.mark.parametrize('width,threads', [(95, 64), (96, 128), (191, 128), (192, 256)])
def test_summary_start_thread_boundaries(width, threads):
    for max_t in (1, 10, 23):
        rc, p = summary_path(S.START, 3, 5, 7, width - 2, 2, 0, max_t, max_t * width, 1, 0)
        assert rc == 0 and (p['kernel'], p['threads'], p['steps']) == (S.K_START, threads, max_t)


def test_signature_dmax_and_fetch_boundaries():
    for d, dmax in [(8, 8), (9, 16), (16, 16), (17, 24), (24, 24), (25, 32), (32, 32)]:
        c = S.C('x', S.SIG, 3, 4, 4, d - 3, 2, 0, 0, 0, depth=3)
        rc, p = summary_path(*S.query_args(c))
        assert rc == 0 and (p['kernel'], p['dmax'], p['threads']) == \
            (S.K_SIG3, dmax, -(-d * d // 64) * 64), d
    # L sd against the thread count: 64 prefetches, 65 is fetched in place (and L ad alike)
    for t, sd, ad, pf in [(16, 4, 3, 1), (13, 5, 2, 0), (16, 3, 4, 1), (13, 2, 5, 0)]:
        rc, p = summary_path(*S.query_args(S.C('x', S.SIG, 3, t, t, sd, ad, 0, 0, 0)))
        assert rc == 0 and (p['threads'], p['prefetch']) == (64, pf), (t, sd, ad)
    # default depth: 3 up to d = 22, 2 from d = 23 (the depth-2 kernel), 1 past d = 110
    for d, kernel, depth in [(22, S.K_SIG3, 3), (23, S.K_SIG12, 2), (110, S.K_SIG12, 2),
                             (111, S.K_SIG12, 1)]:
        rc, p = summary_path(*S.query_args(S.C('x', S.SIG, 3, 5, 5, d - 3, 2, 0, 0, 0)))
        assert rc == 0 and (p['kernel'], p['depth']) == (kernel, depth), d


@pytest.mark.parametrize('name,kind,t,sd,ad,depth,factors', S.REFUSED, ids=[r[0] for r in S.REFUSED])
def test_refused_summary_shapes(name, kind, t, sd, ad, depth, factors):
    """Each refusal: BSIG_EUNSUPPORTED from the query (out all zero) and from the C entry point,
    before it touches the device; one step short of it the shape resolves."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    c = S.C(name, kind, 4, t, t, sd, ad, 0, 0, 0, depth=depth, factors=factors)
    rc, p = summary_path(*S.query_args(c))
    assert rc == _lib.BSIG_EUNSUPPORTED and all(v == 0 for v in p.values()), p
    assert ('LDS' in lib.bsig_last_error().decode()) == ('lds' in name)
    ld = S.pitch(c)
    if kind == S.SIG:
        rc = lib.bsig_signature(fake, fake, fake, 4, t, sd, ad, depth, ld, None)
    elif factors:
        rc = lib.bsig_crosscorr_factors(fake, fake, fake, 4, t, t, sd, ad, 0, ld, None, None)
    else:
        rc = lib.bsig_crosscorr(fake, fake, fake, 4, t, t, sd, ad, 1, ld, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED
    if 'lds' in name:
        smaller = c._replace(t=t - 1) if kind == S.SIG else c._replace(sd=sd - 1)
        rc, p = summary_path(*S.query_args(smaller))
        assert rc == 0 and p['lds'] <= 150 * 1024, p
    else:
        rc, p = summary_path(*S.query_args(c._replace(ad=ad - 1)))
        assert rc == 0 and p['dmax'] == 32


def test_summary_path_argument_errors():
    lib = _lib.load()
    rc, p = summary_path(*S.query_args(S.CASES[0], n=0))
    assert rc == _lib.BSIG_EINVAL and all(v == 0 for v in p.values())
    rc, _ = summary_path(4, 3, 5, 5, 3, 1, 0, 10, 64, 1, 0)
    assert rc == _lib.BSIG_EINVAL and 'kind' in lib.bsig_last_error().decode()
    c = _cc_case(21, 4, 1)
    rc, _ = summary_path(*S.query_args(c._replace(pad=-3)))            # pitch < S A + 2
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in lib.bsig_last_error().decode()
    rc, _ = summary_path(*S.query_args(c._replace(t=1, ta=1)))
    assert rc == _lib.BSIG_EINVAL and 'traj_len' in lib.bsig_last_error().decode()
    assert lib.bsig_debug_summary_path(0, 3, 5, 5, 3, 1, 0, 10, 64, 1, 0, None) == _lib.BSIG_EINVAL


FIT_SCHEDULE_SIZES = list(range(1, 65)) + [100, 101, 104, 1000]


def _fit_schedule(lib, n_updates, step0, n, cap=None):
    cap = 3 + 2 * n_updates if cap is None else cap
    out = (ctypes.c_int32 * max(cap, 1))()
    rc = lib.bsig_debug_fit_schedule(n_updates, step0, n, out, cap)
    return rc, list(out)


def test_fit_schedule_matches_protocol_and_brute_force():
    """The native statement of the chunk protocol's schedule (csrc/fit_protocol.h, through
    bsig_debug_fit_schedule) against protocol.eval_updates and a restatement written here: `every`, the
    logging points, the evaluations before each update, and the evaluations of a launch -- of every
    single-update launch of a call (they add up to the call's) and of the one launch that is the call."""
    from bayes_sim_ig_amd import protocol
    lib = _lib.load()
    for n_updates in FIT_SCHEDULE_SIZES:
        every, its = protocol.eval_updates(n_updates)
        brute_every = n_updates // 5 if n_updates // 5 > 1 else 1
        brute = [it for it in range(n_updates) if it % brute_every == 0 or it == n_updates - 1]
        assert every == brute_every and its == brute
        rc, out = _fit_schedule(lib, n_updates, 0, n_updates)
        assert rc == _lib.BSIG_OK
        assert out[0] == every and out[1] == len(its) and out[2] == len(its)
        assert [it for it in range(n_updates) if out[3 + 2 * it]] == its
        # evaluations before update `it`: those after the updates j < it that the schedule names (the one after
        # the last update follows it, so it precedes no update)
        assert out[4:4 + 2 * n_updates:2] == [sum(1 for j in range(it) if j % every == 0) for it in range(n_updates)]
        total = 0
        for step0 in range(n_updates):
            rc, one = _fit_schedule(lib, n_updates, step0, 1)
            assert rc == _lib.BSIG_OK and one[:2] == out[:2]
            assert one[2] == (1 if step0 in its else 0), (n_updates, step0)
            total += one[2]
        assert total == len(its)


def test_fit_schedule_argument_errors():
    lib = _lib.load()
    assert _fit_schedule(lib, 10, 0, 10)[0] == _lib.BSIG_OK
    assert _fit_schedule(lib, 0, 0, 0, cap=3) == (_lib.BSIG_OK, [1, 0, 0])
    for args in ((-1, 0, 0), (10, -1, 1), (10, 0, -1), (10, 5, 6)):
        assert _fit_schedule(lib, *args, cap=64)[0] == _lib.BSIG_EINVAL, args
    assert _fit_schedule(lib, 10, 0, 10, cap=22)[0] == _lib.BSIG_EINVAL          # 3 + 2 * 10 = 23 needed
    assert 'debug_fit_schedule' in lib.bsig_last_error().decode()
    assert lib.bsig_debug_fit_schedule(10, 0, 10, None, 64) == _lib.BSIG_EINVAL
