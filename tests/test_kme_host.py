"""CPU-side checks of the kernel mean embedding summary (include/bsig_kme.h): the row width, the cover and the
group queries are host arithmetic; every argument check of the launch entry points comes before any launch (the
pattern of tests/test_cabi_errors.py); ``KernelMeanEmbedding`` validates its arguments, draws its frequencies
from a generator of its own and refuses to run before its scale exists, all without a GPU; BayesSim sizes its
first layer by ``kmeFeatures`` and validates its keys.  The numpy restatement of the definition
(tests/kme_cases.py) is checked against a hand-worked two-step example."""
import ctypes as C

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
import kme_cases as KC
from bayes_sim_ig_amd import _lib, summarizers

FAKE = C.c_void_p(4096)      # never dereferenced: validation fails first
CFG = {'modelClass': 'MDNN', 'summarizerFxn': 'summary_kme', 'trainTrajLen': 21, 'components': 3,
       'hiddenLayers': (16, 16), 'lr': 1e-3}
KW = dict(params_dim=2, params_lows=np.array([0.01] * 2), params_highs=np.array([2.0] * 2), prior=None)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsig_last_error().decode()


# ------------------------------------------------------------------ the host queries
@pytest.mark.parametrize('sd,ad', [(3, 1), (60, 8), (48, 12), (211, 20), (1, 1)])
def test_row_width_is_the_closed_form(lib, sd, ad):
    for diff in (0, 1):
        for time in (0, 1):
            want = (2 if diff else 1) * sd + ad + time
            assert KC.row_dim(sd, ad, diff, time) == want == lib.bsig_kme_row_dim(sd, ad, diff, time)
            assert summarizers.kme_row_dim(sd, ad, bool(diff), bool(time)) == want
    assert B.kme_row_dim(sd, ad) == 2 * sd + ad


def test_the_issues_row_widths(lib):
    assert [lib.bsig_kme_row_dim(*dims, 1, 0) for dims in ((3, 1), (60, 8), (211, 20))] == [7, 128, 442]


def test_row_width_refuses_bad_arguments(lib):
    for sd, ad in ((0, 1), (1, 0), (-2, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.bsig_kme_row_dim(sd, ad, 1, 0) == -1
        with pytest.raises(ValueError, match='transition row'):
            summarizers.kme_row_dim(sd, ad)
    for bad in (1.5, '2', None):
        with pytest.raises(ValueError, match='must be ints'):
            summarizers.kme_row_dim(bad, 1)


def test_fits_codes_and_messages(lib):
    ok, einval, eunsup = _lib.BSIG_OK, _lib.BSIG_EINVAL, _lib.BSIG_EUNSUPPORTED
    # (ts, ta, sd, ad, m, diff, time, itemsize)
    assert lib.bsig_kme_fits(21, 21, 3, 1, 128, 1, 0, 4) == ok
    assert lib.bsig_kme_fits(1, 1, 3, 1, 128, 1, 0, 4) == einval and 'M = 0' in err(lib) and 'ts' in err(lib)
    assert lib.bsig_kme_fits(1, 1, 3, 1, 128, 0, 0, 4) == ok               # one state, no difference: M = 1
    assert lib.bsig_kme_fits(2, 1, 3, 1, 128, 1, 1, 8) == ok
    assert lib.bsig_kme_fits(0, 1, 3, 1, 128, 0, 0, 4) == einval and 'ts' in err(lib)
    assert lib.bsig_kme_fits(21, 0, 3, 1, 128, 1, 0, 4) == einval and 'ta' in err(lib)
    assert lib.bsig_kme_fits(21, 21, 0, 1, 128, 1, 0, 4) == einval and 'sd' in err(lib)
    assert lib.bsig_kme_fits(21, 21, 3, 0, 128, 1, 0, 4) == einval and 'ad' in err(lib)
    assert lib.bsig_kme_fits(21, 21, 3, 1, 0, 1, 0, 4) == einval and 'm 0' in err(lib)
    assert lib.bsig_kme_fits(21, 21, 3, 1, -3, 1, 0, 4) == einval and 'm -3' in err(lib)
    assert lib.bsig_kme_fits(21, 21, 3, 1, 128, 1, 0, 2) == einval and 'itemsize' in err(lib)
    # no trajectory is refused for its length: ShadowHand's 119 x 442 fp32 rows are 210 KB as a whole
    for ts in (50, 120, 1000, 100000):
        for itemsize in (4, 8):
            assert lib.bsig_kme_fits(ts, ts, 211, 20, 128, 1, 0, itemsize) == ok
    # only a single block beyond the LDS is: 32 rows of round_up(d, 8) + 1 elements against 160 KiB
    # fp32: d <= 1272 (32 * 1273 * 4 = 162 944 B), double: d <= 632 (32 * 633 * 8 = 162 048 B)
    assert lib.bsig_kme_fits(50, 50, 600, 72, 128, 1, 0, 4) == ok                          # d = 1272
    assert lib.bsig_kme_fits(50, 50, 600, 73, 128, 1, 0, 4) == eunsup and 'LDS' in err(lib)  # d = 1273 -> 1280
    assert lib.bsig_kme_fits(50, 50, 300, 32, 128, 1, 0, 8) == ok                          # d = 632
    assert lib.bsig_kme_fits(50, 50, 300, 33, 128, 1, 0, 8) == eunsup and 'LDS' in err(lib)
    assert lib.bsig_kme_fits(50, 50, 300, 33, 128, 1, 0, 4) == ok


def test_trajectories_per_workgroup(lib):
    """G: for a trajectory of one block (M <= 32) the largest power of two up to 8 whose blocks of
    32 * (round_up(d, 8) + 1) * itemsize bytes take at most 32 KiB together; 1 for a longer one."""
    def want(ts, sd, ad, diff, time, itemsize):
        d = KC.row_dim(sd, ad, diff, time)
        block = KC.BLOCK_ROWS * ((d + 7) // 8 * 8 + 1) * itemsize
        g = 1
        if KC.steps(ts, diff) <= KC.BLOCK_ROWS:
            while g < 8 and 2 * g * block <= 32 * 1024:
                g *= 2
        return g
    assert lib.bsig_kme_group(21, 21, 3, 1, 128, 1, 0, 4) == 8             # 1152 B a block
    assert lib.bsig_kme_group(21, 21, 3, 1, 128, 1, 0, 8) == 8
    assert lib.bsig_kme_group(33, 33, 3, 1, 128, 1, 0, 4) == 8             # M = 32
    assert lib.bsig_kme_group(34, 34, 3, 1, 128, 1, 0, 4) == 1             # M = 33: two blocks
    assert lib.bsig_kme_group(32, 32, 3, 1, 128, 0, 0, 4) == 8 and lib.bsig_kme_group(33, 33, 3, 1, 128, 0, 0, 4) == 1
    assert lib.bsig_kme_group(21, 21, 60, 8, 128, 1, 0, 4) == 1            # 16 512 B a block: two are beyond 32 KiB
    assert lib.bsig_kme_group(21, 21, 12, 6, 128, 1, 0, 4) == 4            # d = 30: 4224 B, eight are 33 792 B
    assert lib.bsig_kme_group(21, 21, 12, 6, 128, 1, 0, 8) == 2
    assert lib.bsig_kme_group(21, 21, 24, 12, 128, 1, 0, 4) == 2           # d = 60: 8320 B
    assert lib.bsig_kme_group(1, 1, 3, 1, 128, 1, 0, 4) == _lib.BSIG_EINVAL
    assert lib.bsig_kme_group(50, 50, 600, 73, 128, 1, 0, 4) == _lib.BSIG_EUNSUPPORTED
    for name, (n, ts, ta, sd, ad, m, diff, time) in KC.CASES.items():
        for itemsize in (4, 8):
            g = lib.bsig_kme_group(ts, ta, sd, ad, m, diff, time, itemsize)
            assert g == want(ts, sd, ad, diff, time, itemsize), name
            assert n is not None or g > 1, name      # the cases that ask for row counts around G share workgroups


@pytest.mark.parametrize('fn', ['bsig_kme', 'bsig_kme_f64'])
def test_launch_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    what = 'kme_f64' if fn.endswith('f64') else 'kme'
    # (states, actions, coeff, ld_coeff, out, n, ts, ta, sd, ad, m, diff, time, ld_out, nonfinite, stream)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 1, 1, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'M = 0' in err(lib) and err(lib).startswith(what + ':')
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 0, 1, 3, 1, 16, 0, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ts' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 0, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ta' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 21, 0, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'sd' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 21, 3, 0, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'ad' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 21, 3, 1, 0, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'm 0' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, 4, 21, 21, 3, 1, 16, 1, 0, 31, None, None)             # width 32
    assert rc == _lib.BSIG_EINVAL and 'ld_out' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 6, FAKE, 4, 21, 21, 3, 1, 16, 1, 0, 32, None, None)             # d = 7
    assert rc == _lib.BSIG_EINVAL and 'ld_coeff' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 7, FAKE, 4, 21, 21, 3, 1, 16, 1, 1, 32, None, None)             # d = 8 with time
    assert rc == _lib.BSIG_EINVAL and 'ld_coeff' in err(lib)
    for args in ((None, FAKE, FAKE, 8, FAKE), (FAKE, None, FAKE, 8, FAKE), (FAKE, FAKE, None, 8, FAKE),
                 (FAKE, FAKE, FAKE, 8, None)):
        rc = call(*args, 4, 21, 21, 3, 1, 16, 1, 0, 32, None, None)
        assert rc == _lib.BSIG_EINVAL and 'null' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 8, FAKE, -1, 21, 21, 3, 1, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EINVAL and 'n=' in err(lib)
    rc = call(FAKE, FAKE, FAKE, 2048, FAKE, 4, 50, 50, 800, 73, 16, 1, 0, 32, None, None)
    assert rc == _lib.BSIG_EUNSUPPORTED and 'LDS' in err(lib)
    # an empty batch is fine and touches nothing, whatever else is passed
    assert call(None, None, None, 0, None, 0, 21, 21, 3, 1, 16, 1, 0, 32, None, None) == _lib.BSIG_OK
    assert call(None, None, None, 0, None, 0, 1, 1, 3, 1, 0, 1, 0, 0, None, None) == _lib.BSIG_OK


@pytest.mark.parametrize('fn', ['bsig_kme_rows', 'bsig_kme_rows_f64'])
def test_rows_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    # (states, actions, rows, n, ts, ta, sd, ad, diff, time, ld_rows, stream)
    assert call(FAKE, FAKE, FAKE, 4, 1, 1, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'M = 0' in err(lib)
    assert call(FAKE, FAKE, FAKE, 4, 0, 1, 3, 1, 0, 0, 8, None) == _lib.BSIG_EINVAL and 'ts' in err(lib)
    assert call(FAKE, FAKE, FAKE, 4, 21, 0, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'ta' in err(lib)
    assert call(FAKE, FAKE, FAKE, 4, 21, 21, 0, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'sd' in err(lib)
    assert call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 0, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'ad' in err(lib)
    assert call(FAKE, FAKE, FAKE, 4, 21, 21, 3, 1, 1, 0, 6, None) == _lib.BSIG_EINVAL and 'ld_rows' in err(lib)
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert call(*args, 4, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'null' in err(lib)
    assert call(FAKE, FAKE, FAKE, -1, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_EINVAL and 'n=' in err(lib)
    assert call(None, None, None, 0, 21, 21, 3, 1, 1, 0, 8, None) == _lib.BSIG_OK


@pytest.mark.parametrize('fn', ['bsig_kme_coeff', 'bsig_kme_coeff_f64'])
def test_coeff_argument_errors_come_before_any_launch(lib, fn):
    call = getattr(lib, fn)
    # (freqs, ld_freqs, inv_std, kappa, coeff, ld_coeff, m, d, stream)
    assert call(FAKE, 7, FAKE, 1.0, FAKE, 8, 0, 7, None) == _lib.BSIG_EINVAL and 'm=0' in err(lib)
    assert call(FAKE, 7, FAKE, 1.0, FAKE, 8, 16, 0, None) == _lib.BSIG_EINVAL and 'd=0' in err(lib)
    assert call(FAKE, 6, FAKE, 1.0, FAKE, 8, 16, 7, None) == _lib.BSIG_EINVAL and 'ld_freqs' in err(lib)
    assert call(FAKE, 7, FAKE, 1.0, FAKE, 6, 16, 7, None) == _lib.BSIG_EINVAL and 'ld_coeff' in err(lib)
    for args in ((None, 7, FAKE, 1.0, FAKE), (FAKE, 7, None, 1.0, FAKE), (FAKE, 7, FAKE, 1.0, None)):
        assert call(*args, 8, 16, 7, None) == _lib.BSIG_EINVAL and 'null' in err(lib)


def test_the_seam_routes_kme(lib):
    for op in ('kme', 'kme_rows', 'kme_coeff'):
        assert _lib.Precision.OPS[op] == ('bsig_' + op, 'bsig_%s_f64' % op)
        assert _lib.F32.symbol(op) == 'bsig_' + op and _lib.F64.symbol(op) == 'bsig_%s_f64' % op
        table = _lib.HEADERS['bsig_kme.h']
        assert table['bsig_' + op] == table['bsig_%s_f64' % op]
    assert set(_lib.HEADERS['bsig_kme.h']) == {
        'bsig_kme_row_dim', 'bsig_kme_fits', 'bsig_kme_group', 'bsig_kme_rows', 'bsig_kme_rows_f64',
        'bsig_kme_coeff', 'bsig_kme_coeff_f64', 'bsig_kme', 'bsig_kme_f64'}
    assert _lib.KME_BLOCK_ROWS == KC.BLOCK_ROWS == 32


# ------------------------------------------------------------------ the numpy definition
def test_the_numpy_reference_is_the_definition_on_a_hand_worked_example():
    """One trajectory, three states of one dimension, two actions (the last one padded... not needed: M = 2),
    one frequency: everything written out."""
    states = np.array([[[1.0], [1.5], [0.5]]], dtype=np.float32)         # differences 0.5, -1.0
    actions = np.array([[[0.25], [-0.75]]], dtype=np.float32)
    coeff = np.array([[2.0, -1.0, 0.5]])                                  # on [s | a | ds]
    x = KC.rows(states, actions, True, False)
    assert x.tolist() == [[[1.0, 0.25, 0.5], [1.5, -0.75, -1.0]]]
    z0, z1 = 2.0 - 0.25 + 0.25, 3.0 + 0.75 - 0.5                          # 2.0, 3.25
    want = [(np.cos(z0) + np.cos(z1)) / 2, (np.sin(z0) + np.sin(z1)) / 2]
    np.testing.assert_allclose(KC.reference(states, actions, coeff, True, False)[0], want, rtol=1e-15)
    # with the time column (tau = 0, 1) and two frequencies: a = sqrt(1/2)
    coeff_t = np.array([[0.5, 2.0, -1.0, 0.5], [-1.0, 0.0, 1.0, 0.0]])
    assert KC.rows(states, actions, True, True)[0, :, 0].tolist() == [0.0, 1.0]
    z = [[z0, 0.25], [0.5 + z1, -1.0 - 0.75]]
    a = np.sqrt(0.5)
    want = [a * (np.cos(z[0][j]) + np.cos(z[1][j])) / 2 for j in range(2)] + \
           [a * (np.sin(z[0][j]) + np.sin(z[1][j])) / 2 for j in range(2)]
    np.testing.assert_allclose(KC.reference(states, actions, coeff_t, True, True)[0], want, rtol=1e-15)
    # without the differences: three rows, the third action padded with the second; tau = 0, 0.5, 1
    x = KC.rows(states, actions, False, True)
    assert x.tolist() == [[[0.0, 1.0, 0.25], [0.5, 1.5, -0.75], [1.0, 0.5, -0.75]]]
    # the fp32 rows are the same values here (all exact), in float32
    x32 = KC.rows(states, actions, False, True, dtype=np.float32)
    assert x32.dtype == np.float32 and np.array_equal(x32, x)
    bound = KC.bounds(states, actions, coeff_t, True, True, 4)
    assert bound.shape == (1, 4) and (bound > 0).all() and (bound < 1e-5).all()
    assert (KC.bounds(states, actions, coeff_t, True, True, 8) < 1e-14).all()


def test_the_coefficient_restatement_and_the_flat_rule():
    freqs = np.array([[1.5, -2.0, 0.25]], dtype=np.float32)
    inv_std = np.array([2.0, 0.0, 1.0 / 3.0])
    got = KC.coefficients(freqs, inv_std, KC.kappa(0.5, 3), np.float32)
    want = [np.float32((1.5 * 2.0) * KC.kappa(0.5, 3)), np.float32(0.0),
            np.float32((0.25 * (1.0 / 3.0)) * KC.kappa(0.5, 3))]
    assert got.dtype == np.float32 and got[0].tolist() == want and got[0, 1] == 0
    assert KC.kappa(0.5, 3) == 1.0 / (0.5 * np.sqrt(3.0))
    x = np.array([[1.0, 5.0], [3.0, 5.0]])
    assert KC.flat_rule_inv_std(x).tolist() == [1.0, 0.0]
    states, actions, freqs, inv_std = KC.case_inputs('constant_action', 9)
    assert inv_std[3] == 0 and (inv_std[[0, 1, 2, 4, 5, 6, 7]] > 0).all()


# ------------------------------------------------------------------ the module
def test_construction_leaves_the_global_generators_alone_and_is_seeded():
    np.random.seed(5), torch.manual_seed(6)
    np_before, torch_before = np.random.get_state(), torch.get_rng_state()
    emb = B.KernelMeanEmbedding(3, 1, n_feat=64, seed=3)
    again = B.KernelMeanEmbedding(3, 1, n_feat=64, seed=3)
    other = B.KernelMeanEmbedding(3, 1, n_feat=64, seed=4)
    np_after = np.random.get_state()
    assert np_before[0] == np_after[0] and np.array_equal(np_before[1], np_after[1]) and np_before[2:] == np_after[2:]
    assert torch.equal(torch_before, torch.get_rng_state())
    assert emb.freqs.dtype == torch.float32 and tuple(emb.freqs.shape) == (32, 7)
    assert torch.equal(emb.freqs, again.freqs) and not torch.equal(emb.freqs, other.freqs)
    want = np.random.RandomState(3).standard_normal((32, 7)).astype(np.float32)
    assert np.array_equal(emb.freqs.numpy(), want)
    assert emb.inv_std.dtype == torch.float64 and tuple(emb.inv_std.shape) == (7,)
    assert emb.count.dtype == torch.int64 and int(emb.count) == 0 and emb.ready is False
    assert sorted(emb.state_dict()) == ['count', 'freqs', 'inv_std']
    assert B.KernelMeanEmbedding(3, 1).n_feat == 256 and B.KernelMeanEmbedding(3, 1).scale == 1.0
    assert tuple(B.KernelMeanEmbedding(3, 1, diff=False, time=True).freqs.shape) == (128, 5)
    given = B.KernelMeanEmbedding(3, 1, n_feat=64, freqs=want * 2)
    assert np.array_equal(given.freqs.numpy(), want * 2)
    emb.double()                                         # the dtypes stay
    assert emb.freqs.dtype == torch.float32 and emb.inv_std.dtype == torch.float64


def test_construction_refuses_bad_arguments():
    for n_feat in (0, 1, 3, 255, -2, 2.0, '4', None, True):
        with pytest.raises(ValueError, match='n_feat'):
            B.KernelMeanEmbedding(3, 1, n_feat=n_feat)
    for scale in (0.0, -1.0, float('inf'), float('nan'), '1', None, True):
        with pytest.raises(ValueError, match='scale'):
            B.KernelMeanEmbedding(3, 1, scale=scale)
    for flag in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='diff'):
            B.KernelMeanEmbedding(3, 1, diff=flag)
        with pytest.raises(ValueError, match='time'):
            B.KernelMeanEmbedding(3, 1, time=flag)
    with pytest.raises(ValueError, match='transition row'):
        B.KernelMeanEmbedding(0, 1)
    with pytest.raises(ValueError, match=r'freqs must be \[n_feat / 2, d\] = \[32, 7\]'):
        B.KernelMeanEmbedding(3, 1, n_feat=64, freqs=np.zeros((32, 8)))


def test_calling_before_the_scale_exists_names_the_remedies():
    emb = B.KernelMeanEmbedding(3, 1, n_feat=16)
    states, actions = torch.zeros(2, 21, 3), torch.zeros(2, 21, 1)
    for call in (lambda: emb(states, actions), lambda: B.summary_kme(states, actions, emb),
                 lambda: emb.coefficients()):
        with pytest.raises(RuntimeError, match='fit_scale.*set_scale.*load_state_dict'):
            call()
    with pytest.raises(ValueError, match='float32 or torch.float64'):
        emb(states, actions, dtype=torch.float16)
    # set_scale and a state_dict make it ready, on the host, without a GPU
    with pytest.raises(ValueError, match='7 values'):
        emb.set_scale(np.ones(6))
    for bad in (-np.ones(7), np.full(7, np.inf), np.full(7, np.nan)):
        with pytest.raises(ValueError, match='finite and >= 0'):
            emb.set_scale(bad)
    emb.set_scale(np.arange(7.0), count=5)
    assert emb.ready and int(emb.count) == 5 and emb.inv_std.tolist() == list(np.arange(7.0))
    twin = B.KernelMeanEmbedding(3, 1, n_feat=16, seed=9)
    assert not twin.ready
    twin.load_state_dict(emb.state_dict())
    assert twin.ready and torch.equal(twin.freqs, emb.freqs) and torch.equal(twin.inv_std, emb.inv_std)
    assert emb.kappa == 1.0 / np.sqrt(7.0)
    with pytest.raises(AssertionError):
        emb(states[0], actions)
    with pytest.raises(AssertionError):
        emb(states[:, :1], actions)                       # one state leaves no difference
    with pytest.raises(AssertionError, match='other dimensions'):
        emb(torch.zeros(2, 21, 4), actions)
    assert B.summary_kme is summarizers.summary_kme and B.bayes_sim.summary_kme is B.summary_kme


# ------------------------------------------------------------------ BayesSim
def _bayes_sim(cfg, obs_dim=3, act_dim=1):
    return B.BayesSim(model_cfg=cfg, obs_dim=obs_dim, act_dim=act_dim, **KW)


def test_bayessim_sizes_its_first_layer_by_the_features():
    bs = _bayes_sim(CFG)
    assert bs.model.input_dim == 256 and bs.summarizer_fxn is B.summary_kme and bs.summarizer_name == 'summary_kme'
    emb = bs.embedding
    assert isinstance(emb, B.KernelMeanEmbedding) and (emb.n_feat, emb.scale, emb.seed) == (256, 1.0, 0)
    assert emb.diff is True and emb.time is False and emb.row_dim == 7 and not emb.ready
    bs = _bayes_sim(dict(CFG, kmeFeatures=64, kmeScale=0.5, kmeSeed=3, kmeDiff=False, kmeTime=True))
    emb = bs.embedding
    assert bs.model.input_dim == 64 and (emb.n_feat, emb.scale, emb.seed, emb.diff, emb.time) == (64, 0.5, 3, False, True)
    assert emb.row_dim == 5 and sorted(emb.state_dict()) == ['count', 'freqs', 'inv_std']
    assert _bayes_sim(dict(CFG, trainTrajLen=120), obs_dim=211, act_dim=20).model.input_dim == 256
    assert _bayes_sim(dict(CFG, trainTrajLen=120, dtype='float64', summaryDtype='float64'), obs_dim=211,
                      act_dim=20).embedding.row_dim == 442


def test_unused_the_embedding_leaves_no_trace():
    torch.manual_seed(3)
    with_kme = _bayes_sim(dict(CFG, kmeFeatures=40))
    torch.manual_seed(3)
    without = _bayes_sim(dict(CFG, summarizerFxn='summary_start'))       # 40 inputs too
    assert without.embedding is None
    assert with_kme.model.input_dim == without.model.input_dim == 40
    a, b = with_kme.model.state_dict(), without.model.state_dict()
    assert list(a) == list(b) and not any('kme' in k or 'embedding' in k for k in a)
    assert all(torch.equal(a[k], b[k]) for k in a)       # the model's draws do not move
    with pytest.raises(RuntimeError, match="without 'summarizerFxn': 'summary_kme'"):
        without.fit_embedding_scale(torch.zeros(2, 21, 3), torch.zeros(2, 21, 1))


def test_bayessim_validates_the_kme_keys():
    for n_feat in (0, 1, 3, -2, 2.0, '4', None, True):
        with pytest.raises(ValueError, match='kmeFeatures'):
            _bayes_sim(dict(CFG, kmeFeatures=n_feat))
    for scale in (0.0, -1.0, 1, '1', None, True, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='kmeScale'):
            _bayes_sim(dict(CFG, kmeScale=scale))
    for seed in (-1, 1.0, '1', None, True, 2 ** 32):
        with pytest.raises(ValueError, match='kmeSeed'):
            _bayes_sim(dict(CFG, kmeSeed=seed))
    for flag in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='kmeDiff'):
            _bayes_sim(dict(CFG, kmeDiff=flag))
        with pytest.raises(ValueError, match='kmeTime'):
            _bayes_sim(dict(CFG, kmeTime=flag))
    defaults = {'kmeFeatures': 256, 'kmeScale': 1.0, 'kmeSeed': 0, 'kmeDiff': True, 'kmeTime': False}
    for other in ('summary_start', 'summary_corrdiff', 'summary_signatory', 'summary_xcorr'):
        for key, value in defaults.items():
            with pytest.raises(ValueError, match="%s.*applies to 'summary_kme'" % key):
                _bayes_sim(dict(CFG, summarizerFxn=other, **{key: value}))
    with pytest.raises(ValueError, match="xcorrLags.*applies to 'summary_xcorr'"):
        _bayes_sim(dict(CFG, xcorrLags=0))
    with pytest.raises(NameError, match="name 'summary_km' is not defined"):
        _bayes_sim(dict(CFG, summarizerFxn='summary_km'))
    with pytest.raises(ValueError, match='trainTrajLen'):
        _bayes_sim(dict(CFG, trainTrajLen=1))
    assert _bayes_sim(dict(CFG, trainTrajLen=1, kmeDiff=False)).embedding.row_dim == 4
    # only a single block of rows beyond a workgroup's LDS is refused
    with pytest.raises(NotImplementedError, match='LDS'):
        _bayes_sim(dict(CFG, trainTrajLen=50), obs_dim=600, act_dim=73)


def test_a_data_parallel_fit_without_a_scale_is_refused_before_any_gpu_call():
    bs = _bayes_sim(dict(CFG, kmeFeatures=16))
    bs.model._dp = object()
    theta, states, actions = torch.zeros(10, 2), torch.zeros(10, 21, 3), torch.zeros(10, 21, 1)
    with pytest.raises(ValueError, match='data-parallel.*fit_embedding_scale'):
        bs._fit_once(theta, states, actions)
    with pytest.raises(ValueError, match='data-parallel.*fit_embedding_scale'):
        bs.run_training(theta, states, actions)
    bs.model._dp = None


def test_the_other_summarizers_keep_their_widths():
    for name, want in (('summary_start', 40), ('summary_corrdiff', 202), ('summary_xcorr', 9)):
        assert _bayes_sim(dict(CFG, summarizerFxn=name)).model.input_dim == want
