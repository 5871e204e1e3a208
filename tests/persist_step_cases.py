"""The step-by-step protocol for the persistent update kernels (csrc/fit_persistent.hip,
csrc/fit_persistent_mdnn.hip + persist_mdnn_device.h, csrc/fit_persistent_mdnn_stream.hip): cases, fp64 / fp32
references and the error bounds.  numpy / torch on the CPU only; tests/test_gpu_persistent_steps.py feeds it what the
kernels left, tests/test_persist_step_host.py checks the protocol itself.

The protocol.  A chunk starts from zeroed Adam moments and leaves them in the model's flat buffers.  The chunk is run
three times from the same start weights w_0 with n_updates = T = 1, 2, 3 and the first T rows of one teacher-forcing
table (EPS_NOISE = 0; with n_updates <= 3 every update logs its training loss and a held-out loss).  Run T gives
(w_T, m_T, v_T, train_loss[0..T), test_loss[0..T)); the logs of run T must begin with the logs of run T - 1 bit for bit
(the prefix property).  Then every update t = 1, 2, 3 is checked BY ITSELF, at the kernel's own previous state:

  1. gradient      g_t = m_{t-1} + (m_t - m_{t-1}) / ob1, recovered in double from the fp32 moments, against the fp64
                   gradient (oracle/estimators.py under torch.set_default_dtype(float64)) at the kernel's own w_{t-1},
                   widened exactly, on the rows ids[t-1];
  2. second moment v_t against ob2 g_t^2 + b2f v_{t-1}, evaluated in double from the recovered g_t;
  3. weight step   w_t against w_{t-1} - a0(t) m_t / (sqrt(v_t) a1(t) + eps) from the kernel's own m_t, v_t, w_{t-1},
                   every element, a0(t) = lr / (1 - beta1^t) and a1(t) = 1 / sqrt(1 - beta2^t) computed in double;
  4. training loss train_loss[t-1] against the fp64 mean NLL at w_{t-1} on the rows ids[t-1];
  5. held-out loss test_loss[t-1] against the fp64 mean NLL at w_t on the held-out rows;
  6. padding       every stored element outside the parameters' views: m, v and w exactly zero.

The hyper-parameters are the ones the C ABI carries: bsig_mdn_cfg holds lr, beta1, beta2 and adam_eps as fp32 fields,
so the Adam the kernels are given is the one with beta1 = float32(0.9), beta2 = float32(0.999), lr = float32(1e-3),
eps = float32(1e-8), each widened exactly (HYPER below).  ob1 = 1 - beta1, ob2 = 1 - beta2 and b2f = beta2 are exact in
fp32 (persist_device.h: AdamK).  Items 2 and 3 hold the kernels to THAT Adam, with the powers beta^t taken by `**` in
double and not by the running products of fit_protocol.h: adam_advance.

Derived bounds (u = 2^-24, the unit roundoff of fp32; first order in u, every bound carries a factor 1 + 2^-10 for the
higher orders; TINY = 2^-126 covers results flushed below the normal range).

  Recovery of g.  adam_weight / adam_bias: m_t = fl(fma(fl(g - m'), ob1, m')), m' = m_{t-1}: two roundings,
      m_t = ((g - m')(1 + d1) ob1 + m')(1 + d2).  With ghat = m' + (m_t - m') / ob1 in double:
      |ghat - g| <= E_g = (u |m_t| + u |m_t - m'|) / ob1 + TINY / ob1.
    Relative to the largest gradient G of the tensor (|m| <= G, |m_t - m'| <= ob1 (|g| + |m'|) <= 2 ob1 G) that is at most
    (2 + 1 / ob1) u; the floor used for item 1 is the rounder R_FLOOR = (2 + 2 / ob1) u = 22 u = 1.3e-6, which covers it.

  Item 2.  v_t = fl(fma(fl(ob2 g), g, fl(v' b2f))): three roundings, each relative to its own (non-negative) term,
      |v_t - (ob2 g^2 + b2f v')| <= u ob2 g^2 + u b2f v' + u v_t,
    and evaluating the reference at ghat instead of g adds ob2 (2 |ghat| E_g + E_g^2); g^2 <= (|ghat| + E_g)^2.

  Item 3, weights (adam_weight).  s = v_sqrt_f32(v) (1 ulp = 2 u), a1 as a float (u), eps as a float (u), the fma
    d = fl(s a1 + eps) (u): both terms are non-negative, so d = D (1 + 4 u), D = sqrt(v) a1 + eps in double.  r =
    v_rcp_f32(d) (2 u): 6 u.  p = fl(m r) (u): 7 u.  a0 as a float (u): 8 u on S = a0 m / D.  The last fma rounds once:
      |w_t - (w' - S)| <= 8 u |S| + u |w_t|.
  Item 3, biases (adam_bias).  IEEE sqrtf (u) and a1 (u) act on the first term of the sum, the rounding of eps (u) on the
    second: the sum is off by max(2 u, u), the fma by one more: d = D (1 + 3 u); IEEE division (u): 4 u; a0 (u): 5 u:
      |w_t - (w' - S)| <= 5 u |S| + u |w_t|.

Measured margins (items 1, 4, 5; the yardstick is the fp32 oracle on the CPU at the same weights, rows and inputs, never
the code under test).  Per tensor q = max |g_kernel - g64| / max |g64| and r the same figure of the fp32 oracle;
the test asserts q <= M_GRAD max(r, R_FLOOR).  Losses: q = |L_kernel - L64| / mean_i |l_i| with l_i the fp64 NLL of
row i (a mean of B fp32 terms is off by at most (B + 1) u mean |l_i|: B - 1 additions, the rounding of a term, the
division), r the same figure of the fp32 oracle, floor (B + 1) u; q <= M_LOSS max(r, floor).  The margins are fixed
from the first GPU run by the rule of tests/test_gpu_persistent_steps.py (smallest power of two >= 2 x the worst
ratio seen, never above M_CAP = 16).

The jitter path (EPS_NOISE = 1e-5) has no fp64 reference of the device RNG; it is compared kernel against kernel
(persistent against per-phase, same streams) by the same rule with BOTH gradients recovered: floor 2 R_FLOOR."""
import contextlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
M_CAP = 16.0
N_STEPS = 3
MODEL_SEED, DATA_SEED, IDS_SEED = 77, 3, 5
F32 = np.float32


class Hyper:
    """The Adam the kernels are given: the fp32 fields of bsig_mdn_cfg, widened exactly."""

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps = (float(F32(v)) for v in (lr, beta1, beta2, eps))
        self.ob1 = float(F32(1.0) - F32(beta1))       # AdamK: 1.0f - (float)beta1, exact in fp32
        self.ob2 = float(F32(1.0) - F32(beta2))
        self.b2f = float(F32(beta2))
        assert self.ob1 == 1.0 - self.b1 and self.ob2 == 1.0 - self.b2

    def a0(self, t):
        return self.lr / (1.0 - self.b1 ** t)

    def a1(self, t):
        return 1.0 / math.sqrt(1.0 - self.b2 ** t)


HYPER = Hyper()
R_FLOOR = (2.0 + 2.0 / HYPER.ob1) * U


def loss_floor(n_rows):
    return (n_rows + 1.0) * U


# ---------------------------------------------------------------------------------- Adam: recovery, references, bounds
def recover_gradient(m_prev, m_t, hy=HYPER):
    """(ghat, E_g): the gradient the kernel fed its first moment, in double, and the bound on |ghat - g|."""
    m_prev, m_t = np.asarray(m_prev, np.float64), np.asarray(m_t, np.float64)
    ghat = m_prev + (m_t - m_prev) / hy.ob1
    e_g = SLACK * (U * np.abs(m_t) + U * np.abs(m_t - m_prev) + TINY) / hy.ob1
    return ghat, e_g


def second_moment(ghat, e_g, v_prev, v_t, hy=HYPER):
    """(reference, bound) of item 2, elementwise."""
    v_prev, v_t = np.asarray(v_prev, np.float64), np.asarray(v_t, np.float64)
    ref = hy.ob2 * ghat * ghat + hy.b2f * v_prev
    g_hi = np.abs(ghat) + e_g
    bound = SLACK * (U * hy.ob2 * g_hi * g_hi + U * hy.b2f * v_prev + U * np.abs(v_t) + 3 * TINY
                     + hy.ob2 * (2.0 * np.abs(ghat) * e_g + e_g * e_g))
    return ref, bound


def weight_step(w_prev, m_t, v_t, w_t, t, is_bias, hy=HYPER):
    """(reference, bound) of item 3, elementwise, from the kernel's own moments."""
    w_prev, m_t, v_t, w_t = (np.asarray(a, np.float64) for a in (w_prev, m_t, v_t, w_t))
    d = np.sqrt(v_t) * hy.a1(t) + hy.eps
    s = hy.a0(t) * m_t / d
    n_u = 5.0 if is_bias else 8.0
    bound = SLACK * (n_u * U * np.abs(s) + U * np.abs(w_t) + 2 * TINY)
    return w_prev - s, bound


def adam_replay64(w, grads, hy):
    """torch's Adam in double, operation by operation: the weights after each of the gradients (w fixed shape)."""
    w = np.asarray(w, np.float64).copy()
    m, v, out = np.zeros_like(w), np.zeros_like(w), []
    for t, g in enumerate(grads, 1):
        m = m + (g - m) * hy.ob1
        v = hy.b2f * v + hy.ob2 * g * g
        w = w - hy.a0(t) * m / (np.sqrt(v) * hy.a1(t) + hy.eps)
        out.append((w.copy(), m.copy(), v.copy()))
    return out


def _fma32(a, b, c):
    """fl32(a b + c) of float32 arrays: the product of two floats is exact in double; the sum is rounded to double and
    then to float (a double rounding only on exact ties of the 29 spare bits: not on random data)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _ulp_off(x, k):
    """x moved by k (array of -1, 0, 1) units in the last place"""
    bits = x.astype(F32).view(np.int32) + k.astype(np.int32)
    return np.where((x == 0) | ~np.isfinite(x), x, bits.view(F32)).astype(F32)


def emulate_adam(g, m, v, w, t, is_bias, hy=HYPER, rng=None):
    """adam_weight / adam_bias of persist_device.h on float32 arrays: -> (m_t, v_t, w_t).  The weight path's
    v_sqrt_f32 and v_rcp_f32 are the correctly rounded values moved by a random -1 / 0 / +1 ulp (`rng`)."""
    g, m, v, w = (np.asarray(a, F32) for a in (g, m, v, w))
    ob1, ob2, b2f, eps = F32(hy.ob1), F32(hy.ob2), F32(hy.b2f), F32(hy.eps)
    a0, a1 = F32(hy.a0(t)), F32(hy.a1(t))
    ones = np.ones_like(g)
    m_t = _fma32((g - m).astype(F32), ob1 * ones, m)
    v_t = _fma32((ob2 * g).astype(F32), g, (v * b2f).astype(F32))
    sq = np.sqrt(v_t.astype(np.float64)).astype(F32)
    if is_bias:
        w_t = _fma32(-a0 * ones, (m_t / _fma32(sq, a1 * ones, eps * ones)).astype(F32), w)
    else:
        jit = (lambda x: _ulp_off(x, rng.randint(-1, 2, x.shape))) if rng is not None else (lambda x: x)
        d = _fma32(jit(sq), a1 * ones, eps * ones)
        r = jit((1.0 / d.astype(np.float64)).astype(F32))
        w_t = _fma32(-a0 * ones, (m_t * r).astype(F32), w)
    return m_t, v_t, w_t


# ------------------------------------------------------------------------------------------------------------- cases
def _mdrff(d, k, n_feat, n, batch, **kw):
    return dict(kind='MDRFF', d=d, k=k, n_feat=n_feat, n=n, batch=batch, summarizer='summary_start', t=11, sd=5, ad=2,
                hidden=[], engine=1, **kw)


def _mdnn(d, k, batch=100, n=1000, summarizer='summary_start', t=11, sd=5, ad=2, hidden=(128, 128), **kw):
    return dict(kind='MDNN', d=d, k=k, n_feat=0, n=n, batch=batch, summarizer=summarizer, t=t, sd=sd, ad=ad,
                hidden=list(hidden), engine=2, **kw)


# geom: what bsig_debug_persist_geometry / bsig_debug_persist_mdnn_geometry must report for the case (the names of
# tests/test_host_logic.py).  Linear heads: 16-row head blocks, k-slices of 96 features.
CASES = {
    # Nh = 35 -> three head blocks (the last one ragged), 512 features -> six k-slices (the last one ragged)
    'lin_blocks_x_slices': _mdrff(3, 5, 512, 1000, 100, geom=dict(NT=1, n_blocks=3, k_slices=6, n_owner=100, R=1)),
    'lin_eval_in_launch': _mdrff(3, 5, 512, 1000, 100, env={'BSIG_EVAL_IN_LAUNCH': '1'}, in_launch=True,
                                 geom=dict(NT=1, n_blocks=3, k_slices=6, n_owner=100, R=1)),
    'lin_generic_rows': _mdrff(3, 5, 512, 1000, 100, env={'BSIG_PERSIST_FAST_ROWS': '0'},
                               geom=dict(NT=1, n_blocks=3, k_slices=6, n_owner=100, R=1)),
    # Nh = 50: a padded row in the fourth block; 200 = 2 x 96 + 8: masked k tail
    'lin_padded_row_k_tail': _mdrff(2, 10, 200, 1000, 100, geom=dict(NT=1, n_blocks=4, k_slices=3, n_owner=100, R=1)),
    # batch below a tile, 48 training rows, 12 held-out rows
    'lin_small_batch': _mdrff(3, 4, 256, 60, 7, geom=dict(NT=1, n_blocks=2, k_slices=3, n_owner=7, R=1, NE=6, RE=2)),
    # a batch larger than the training split (48 rows): every row repeated
    'lin_batch_over_split': _mdrff(3, 5, 512, 60, 100, geom=dict(NT=1, n_blocks=3, k_slices=6, n_owner=100, R=1)),
    # I = 70: one ragged k-slice of 256
    'mdnn_one_slice': _mdnn(3, 5, geom=dict(k_slices=1, G1=4, mr=1, n_owner=100, wide=0, stream=0, Nh=35)),
    # I = 3 x 10 x 3 x 8 + 2 = 722 (I % 4 = 2): three k-slices
    'mdnn_three_slices': _mdnn(17, 5, summarizer='summary_corrdiff', t=3, sd=11, ad=8, input_dim=722,
                               geom=dict(k_slices=3, G1=12, mr=1, n_owner=100, wide=0, stream=0, Nh=175)),
    'mdnn_full_cov_odd_batch': _mdnn(3, 4, batch=10, full=True,
                                     geom=dict(k_slices=1, mr=4, n_owner=3, wide=0, stream=0, Nh=40)),
    'mdnn_smallest_batch': _mdnn(3, 5, batch=3, n=5, geom=dict(k_slices=1, mr=1, n_owner=3, wide=0, stream=0)),
    'mdnn_single_input': _mdnn(3, 5, column=63, input_dim=1, geom=dict(k_slices=1, mr=1, n_owner=100, stream=0)),
    'mdnn_padded_trunk': _mdnn(2, 10, t=21, sd=3, ad=1, hidden=(24, 24), input_dim=40,
                               geom=dict(k_slices=1, mr=1, n_owner=100, wide=0, stream=0, Nh=50)),
    'mdnn_forced_wide': _mdnn(3, 5, env={'BSIG_MDNN_WIDE_HEADS': '1'},
                              geom=dict(k_slices=1, mr=1, n_owner=100, wide=1, stream=0, Nh=35)),
    # (BSIG_MDNN_MR is read once per process: these two run in a fresh child process each)
    'mdnn_two_rows': _mdnn(3, 5, env={'BSIG_MDNN_MR': '2'}, child=True,
                           geom=dict(k_slices=1, mr=2, n_owner=50, wide=0, stream=0)),
    'mdnn_four_rows': _mdnn(3, 5, env={'BSIG_MDNN_MR': '4'}, child=True,
                            geom=dict(k_slices=1, mr=4, n_owner=25, wide=0, stream=0)),
    # the SMALL shape of tests/test_gpu_persistent_stream.py: S = 8 x 20, A = 8 x 12, I = 15362, factor rows
    'stream_batch_100': _mdnn(3, 5, summarizer='summary_corrdiff', t=8, sd=21, ad=12, lazy=True, input_dim=15362,
                              geom=dict(k_slices=61, mr=8, n_owner=13, wide=0, stream=1)),
    'stream_ragged_batch': _mdnn(3, 5, batch=37, summarizer='summary_corrdiff', t=8, sd=21, ad=12, lazy=True,
                                 input_dim=15362, geom=dict(k_slices=61, mr=8, n_owner=5, wide=0, stream=1)),
}
JITTER_CASES = ('lin_blocks_x_slices', 'mdnn_one_slice')
LIN_GEOM = ['NT', 'KS', 'n_blocks', 'k_slices', 'G', 'T', 'n_owner', 'R', 'NE', 'RE', 'eval_passes', 'lds', 'mixed',
            'kernel']
MDNN_GEOM = ['k_slices', 'G1', 'n_owner', 'mr', 'n_small', 'wide', 'stream', 'eval_passes', 'lds', 'Nh']


def shape_key(spec):
    """What the references depend on: cases that differ in switches only share them."""
    return tuple((k, repr(spec.get(k))) for k in ('kind', 'd', 'k', 'n_feat', 'n', 'batch', 'summarizer', 't', 'sd',
                                                  'ad', 'hidden', 'full', 'column', 'lazy'))


def bench_cfg(spec):
    return dict(task='synthetic', model=spec['kind'], summarizer=spec['summarizer'], t=spec['t'], sd=spec['sd'],
                ad=spec['ad'], d=spec['d'], k=spec['k'], hidden=list(spec['hidden']), n_feat=spec['n_feat'],
                pairs=spec['n'], full=bool(spec.get('full', False)))


def split(spec):
    n_train = max(int(spec['n'] * 0.8), 1)
    return n_train, spec['n'] - n_train


def case_ids(spec):
    """ids[3, batch]: seeded draws from the training split, with a duplicate in every minibatch."""
    ids = np.random.RandomState(IDS_SEED).randint(0, split(spec)[0], (N_STEPS, spec['batch']))
    if spec['batch'] >= 2:
        ids[:, 1] = ids[:, 0]
    return ids


def case_data(spec):
    """(theta, states, actions) on the CPU (bench.synth_pairs): the same bits wherever the case runs."""
    import bench
    return bench.synth_pairs(bench_cfg(spec), spec['n'], DATA_SEED, 'cpu')


def build_model(pkg, spec, device):
    """(BayesSim, model) as the neighbouring tests build them (bench.build_gpu_model, seed 77); the single-input case
    takes one column of the summary into a model of its own."""
    import bench
    bs = bench.build_gpu_model(pkg, bench_cfg(spec), device, MODEL_SEED)
    if spec.get('column') is None:
        return bs, bs.model
    torch.manual_seed(MODEL_SEED)
    d = spec['d']
    model = pkg.MDNN(input_dim=1, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d),
                     n_gaussians=spec['k'], full_covariance=bool(spec.get('full', False)),
                     hidden_layers=tuple(spec['hidden']), activation=torch.nn.Tanh, lr=1e-3, device=device)
    return bs, model


def param_views(model, flat):
    """{name: float64 array} of the parameters' views of a flat buffer (numpy, the model's layout) and the mask of the
    stored elements outside every view."""
    flat = np.asarray(flat)
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == len(model._param_slices)
    out, mask = {}, np.ones(flat.shape, bool)
    for name, (o, full, real) in zip(names, model._param_slices):
        size = int(np.prod(full))
        sub = tuple(slice(0, r) for r in real)
        out[name] = flat[o:o + size].reshape(full)[sub].astype(np.float64)
        mask[o:o + size].reshape(full)[sub] = False
    return out, mask


# ------------------------------------------------------------------------------------------------------- references
@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def rows_from_factors(sf, af, mean, std, dtype):
    """The cross-correlation summary rows [outer(sf, af) | mean | std] of fp32 factors, formed in `dtype` (in double the
    products of two floats are exact; in float each is the one fp32 multiply the kernels do)."""
    sf, af = sf.to(dtype), af.to(dtype)
    outer = (sf.unsqueeze(2) * af.unsqueeze(1)).reshape(sf.shape[0], -1)
    return torch.cat([outer, mean.to(dtype).reshape(-1, 1), std.to(dtype).reshape(-1, 1)], dim=1)


class Reference:
    """oracle/estimators.py at given weights on given rows, in float64 (the reference) and float32 (the yardstick).
    `x`: the fp32 rows the kernels consume ([n, I] tensor), or (sf, af, mean, std) fp32 factors; `y`: fp32 targets
    [n, d] in the unit box (lows 0, highs 1: the kernels' normalisation is exact); `coeff`: an MDRFF's fp32
    frequencies / sigma [n_feat / 2, I] as the projection takes them."""

    def __init__(self, spec, x, y, coeff=None):
        self.spec, self.coeff = spec, coeff
        self.x = {}
        for dt in (torch.float64, torch.float32):
            self.x[dt] = rows_from_factors(*x, dtype=dt) if isinstance(x, tuple) else x.detach().cpu().to(dt)
        self.y = {dt: y.detach().cpu().to(dt) for dt in (torch.float64, torch.float32)}
        self.input_dim = self.x[torch.float64].shape[1]
        self._oracles = {}

    def _oracle(self, dtype):
        if dtype not in self._oracles:
            from oracle import estimators as oest
            s, d = self.spec, self.spec['d']
            kw = dict(input_dim=self.input_dim, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d),
                      n_gaussians=s['k'], full_covariance=bool(s.get('full', False)), lr=1e-3,
                      activation=torch.nn.Tanh, eps_noise=0.0)
            with default_dtype(dtype):
                if s['kind'] == 'MDRFF':
                    o = oest.OracleMDRFF(n_feat=s['n_feat'], sigma=1.0, freqs=self.coeff.detach().cpu().numpy(), **kw)
                    o.rff.freqs, o.rff.sigma = o.rff.freqs.to(dtype), o.rff.sigma.to(dtype)
                else:
                    o = oest.OracleMDNN(hidden_layers=list(s['hidden']), **kw)
            self._oracles[dtype] = o
        return self._oracles[dtype]

    def _loaded(self, state, dtype):
        o = self._oracle(dtype)
        o.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items()})
        return o

    def grad(self, state, rows, dtype=torch.float64):
        """(mean NLL, {name: gradient}) at `state` ({name: array}, fp32 values) on the rows `rows` (repeats count)."""
        with default_dtype(dtype):
            o = self._loaded(state, dtype)
            o.zero_grad()
            rows = torch.as_tensor(np.asarray(rows), dtype=torch.long)
            loss = o.mdn_loss_fn(*o.forward(self.x[dtype][rows]), self.y[dtype][rows])
            loss.backward()
            return float(loss.item()), {k: p.grad.detach().double().numpy().copy() for k, p in o.named_parameters()}

    def loss(self, state, rows, dtype=torch.float64):
        with default_dtype(dtype), torch.no_grad():
            o = self._loaded(state, dtype)
            rows = torch.as_tensor(np.asarray(rows), dtype=torch.long)
            return float(o.mdn_loss_fn(*o.forward(self.x[dtype][rows]), self.y[dtype][rows]).item())

    def row_nll(self, state, rows):
        """The fp64 NLL of every row (the closed form of oracle/estimators.py, a second evaluation)."""
        from oracle import estimators as oest
        with default_dtype(torch.float64), torch.no_grad():
            o = self._loaded(state, torch.float64)
            rows = torch.as_tensor(np.asarray(rows), dtype=torch.long)
            w, mu, l_d, low = o.forward(self.x[torch.float64][rows])
            logp = oest._component_logp(self.y[torch.float64][rows].numpy(), mu.numpy(), l_d.numpy(),
                                        None if low is None else low.numpy(), self.spec['d'])[0]
            return -oest._mixture_nll(logp, w.numpy(), len(rows), oest.MIN_WEIGHT, oest.LL_LIMIT)[1]


def host_reference(pkg, spec):
    """(Reference, start weights {name: fp32 array}) of a case without a GPU: the model built on the CPU (the same
    seeded initialisation), the oracle's summaries of the same pairs."""
    from oracle import summarize as osum
    theta, states, actions = case_data(spec)
    _, model = build_model(pkg, spec, 'cpu')
    coeff = None
    if spec.get('lazy'):
        sf, af = osum.crosscorr_features(states, actions, use_state_diff=True)
        x = (sf, af, sf.mean(dim=-1), sf.std(dim=-1))
    else:
        x = osum.SUMMARIZERS[spec['summarizer']](states, actions)
        if spec.get('column') is not None:
            x = x[:, spec['column']:spec['column'] + 1].contiguous()
    if spec['kind'] == 'MDRFF':
        coeff = (model.rff.freqs.cpu() / model.rff.sigma.cpu()).float()
    state0 = {k: v.detach().cpu().numpy().astype(F32) for k, v in model.named_parameters()}
    return Reference(spec, x, theta, coeff), state0


def rel_err(a, ref):
    """max |a - ref| / max |ref|"""
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ the protocol itself
def check_prefix(runs):
    """The logs of run T begin with the logs of run T - 1, bit for bit."""
    for a, b in zip(runs[:-1], runs[1:]):
        for key in ('train_loss', 'test_loss'):
            pa, pb = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)[:len(a[key])]
            assert len(a[key]) + 1 == len(b[key]) and pa.tobytes() == pb.tobytes(), ('prefix property', key, pa, pb)


def check_steps(model, ref, w0_flat, runs, ids, n_test, hy=HYPER):
    """Items 1-6 on the runs T = 1, 2, 3 of one case.  `runs[T-1]` = dict(w, m, v: flat fp32 numpy arrays after run T,
    train_loss, test_loss: its logs).  Asserts the prefix property, the padding and the derived bounds (items 2, 3);
    returns the figures of the measured items for the caller to print and assert:
      grad[(t, name)] = (q, r), train[t] / test[t] = (q, r, floor), adam = worst |error| / bound of items 2 and 3."""
    check_prefix(runs)
    n_train = ref.x[torch.float64].shape[0] - n_test
    held = np.arange(n_train, n_train + n_test)
    batch = ids.shape[1]
    zeros = np.zeros_like(np.asarray(w0_flat))
    prev = dict(w=np.asarray(w0_flat), m=zeros, v=zeros)
    out = dict(grad={}, train={}, test={}, adam=dict(v=0.0, w=0.0), recovery={}, scale={})
    for t, run in enumerate(runs, 1):
        w_prev, mask = param_views(model, prev['w'])
        (m_prev, _), (v_prev, _) = param_views(model, prev['m']), param_views(model, prev['v'])
        (w_t, _), (m_t, _), (v_t, _) = (param_views(model, run[k]) for k in ('w', 'm', 'v'))
        for k in ('w', 'm', 'v'):                                                       # item 6
            assert not np.asarray(run[k])[mask].any(), ('padding not zero', k, t)
        # fp32 values: the widening is exact, and float32 holds them again for the fp32 oracle
        state_prev = {k: v.astype(F32) for k, v in w_prev.items()}
        state_t = {k: v.astype(F32) for k, v in w_t.items()}
        l64, g64 = ref.grad(state_prev, ids[t - 1], torch.float64)
        l32, g32 = ref.grad(state_prev, ids[t - 1], torch.float32)
        for name in w_t:
            is_bias = w_t[name].ndim == 1
            ghat, e_g = recover_gradient(m_prev[name], m_t[name], hy)
            out['grad'][(t, name)] = (rel_err(ghat, g64[name]), rel_err(g32[name], g64[name]))       # item 1
            out['recovery'][(t, name)] = float(e_g.max() / max(np.abs(g64[name]).max(), 1e-300))
            v_ref, v_bound = second_moment(ghat, e_g, v_prev[name], v_t[name], hy)                   # item 2
            out['adam']['v'] = max(out['adam']['v'], float((np.abs(v_t[name] - v_ref) / v_bound).max()))
            w_ref, w_bound = weight_step(w_prev[name], m_t[name], v_t[name], w_t[name], t, is_bias, hy)   # item 3
            out['adam']['w'] = max(out['adam']['w'], float((np.abs(w_t[name] - w_ref) / w_bound).max()))
        nll = ref.row_nll(state_prev, ids[t - 1])                                                    # item 4
        scale = float(np.abs(nll).mean())
        assert abs(nll.mean() - l64) <= 1e-10 * scale, ('the two fp64 evaluations of the loss disagree', nll.mean(), l64)
        out['scale'][('train', t)] = scale
        out['train'][t] = (abs(run['train_loss'][t - 1] - l64) / scale, abs(l32 - l64) / scale, loss_floor(batch))
        if n_test > 0:                                                                               # item 5
            t64, t32 = ref.loss(state_t, held, torch.float64), ref.loss(state_t, held, torch.float32)
            scale = float(np.abs(ref.row_nll(state_t, held)).mean())
            out['scale'][('test', t)] = scale
            out['test'][t] = (abs(run['test_loss'][t - 1] - t64) / scale, abs(t32 - t64) / scale, loss_floor(n_test))
        prev = run
    return out


def worst_ratios(res):
    """(gradient, loss) worst q / max(r, floor) of a check_steps result"""
    g = max(q / max(r, R_FLOOR) for q, r in res['grad'].values())
    ls = max(q / max(r, fl) for q, r, fl in list(res['train'].values()) + list(res['test'].values()))
    return g, ls


def describe(name, res):
    g, ls = worst_ratios(res)
    lines = ['%s: Adam worst |error| / bound: v %.3f, w %.3f; gradient worst q / max(r, floor) %.3f; loss %.3f'
             % (name, res['adam']['v'], res['adam']['w'], g, ls)]
    for (t, tensor), (q, r) in sorted(res['grad'].items()):
        lines.append('    t=%d %-18s q %.3e  r %.3e  q/max(r,floor) %.3f' % (t, tensor, q, r, q / max(r, R_FLOOR)))
    for key in ('train', 'test'):
        for t, (q, r, fl) in sorted(res[key].items()):
            lines.append('    t=%d %-18s q %.3e  r %.3e  floor %.3e  q/max(r,floor) %.3f'
                         % (t, key + '_loss', q, r, fl, q / max(r, fl)))
    return '\n'.join(lines)
