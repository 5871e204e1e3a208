"""The step-by-step protocol of tests/persist_step_cases.py, checked without a GPU: the fp64 Adam replay against
torch.optim.Adam in double, the recovery algebra and the derived bounds of items 2 and 3 on a float32 emulation of
adam_weight / adam_bias (persist_device.h), and the sensitivity condition -- for every case, the gradient error the GPU
test may allow at the cap M = 16 is at most a quarter of what each of four plausible kernel mistakes changes."""
import numpy as np
import pytest
import torch

import persist_step_cases as PS

HY = PS.HYPER


def test_hyper_parameters_are_the_kernels_floats():
    """AdamK of persist_device.h: ob1 = 1.0f - (float)beta1, b2f = (float)beta2, ob2 = 1.0f - (float)beta2; the
    differences are exact in fp32, and R_FLOOR is 22 u."""
    f = np.float32
    assert HY.ob1 == float(f(1) - f(0.9)) and HY.ob2 == float(f(1) - f(0.999)) and HY.b2f == float(f(0.999))
    assert HY.ob1 + HY.b1 == 1.0 and HY.ob2 + HY.b2 == 1.0
    assert abs(PS.R_FLOOR / PS.U - 22.0) < 1e-4
    # the powers by ** against the running products of fit_protocol.h: adam_advance, as floats
    b1t = b2t = 1.0
    for t in (1, 2, 3):
        b1t, b2t = b1t * HY.b1, b2t * HY.b2
        assert f(HY.lr / (1.0 - b1t)) == f(HY.a0(t)) and f(1.0 / np.sqrt(1.0 - b2t)) == f(HY.a1(t))


def test_fp64_replay_equals_torch_adam_in_double():
    rng = np.random.RandomState(0)
    w0 = rng.randn(257)
    grads = [rng.randn(257) * s for s in (1.0, 1e-3, 10.0)]
    grads[1][:5] = 0.0
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=HY.lr, betas=(HY.b1, HY.b2), eps=HY.eps)
    for (w, m, v), g in zip(PS.adam_replay64(w0, grads, HY), grads):
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        for got, ref in ((w, p.detach().numpy()), (m, st['exp_avg'].numpy()), (v, st['exp_avg_sq'].numpy())):
            assert np.abs(got - ref).max() <= 1e-14 * max(np.abs(ref).max(), 1e-300)
    # ... and the item-3 reference is that step: from torch's own moments it gives torch's weights
    st = opt.state[p]
    w2 = PS.adam_replay64(w0, grads, HY)[1][0]
    ref, _ = PS.weight_step(w2, st['exp_avg'].numpy(), st['exp_avg_sq'].numpy(), p.detach().numpy(), 3, False, HY)
    assert np.abs(ref - p.detach().numpy()).max() <= 1e-14


def _emulated_ratios(is_bias, wrong=None, seed=1):
    """Three emulated fp32 steps on gradients of every size: worst |error| / bound of the recovery, item 2, item 3."""
    rng = np.random.RandomState(seed)
    n = 4096
    w = rng.randn(n).astype(np.float32) * 0.1
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    worst = dict(g=0.0, v=0.0, w=0.0)
    for t in (1, 2, 3):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-9, 1, n)).astype(np.float32)
        g[:64] = 0.0
        g[64:128] = (rng.randn(64) * 1e-9).astype(np.float32)
        hy = PS.Hyper()
        if wrong == 'a1':                  # the bias correction of the second moment one step ahead
            hy.a1 = lambda tt, a1=hy.a1: a1(tt + 1)
        g_fed = g * np.float32(1.01) if wrong == 'v' else g      # (a second moment fed another gradient)
        m_t, v_t, w_t = PS.emulate_adam(g, m, v, w, t, is_bias, hy, rng)
        if wrong == 'v':
            v_t = PS.emulate_adam(g_fed, m, v, w, t, is_bias, hy, rng)[1]
        ghat, e_g = PS.recover_gradient(m, m_t)
        worst['g'] = max(worst['g'], float((np.abs(ghat - g.astype(np.float64)) / e_g).max()))
        v_ref, v_b = PS.second_moment(ghat, e_g, v, v_t)
        worst['v'] = max(worst['v'], float((np.abs(v_t - v_ref) / v_b).max()))
        w_ref, w_b = PS.weight_step(w, m_t, v_t, w_t, t, is_bias)
        worst['w'] = max(worst['w'], float((np.abs(w_t - w_ref) / w_b).max()))
        m, v, w = m_t, v_t, w_t
    return worst


@pytest.mark.parametrize('is_bias', [False, True])
def test_recovery_and_bounds_hold_for_emulated_fp32_adam(is_bias):
    """g = 0, |g| ~ 1e-9 and sizes up to 10: the recovered gradient within E_g, items 2 and 3 within their bounds --
    and not by a wide margin: the worst case uses a fair part of each bound."""
    worst = _emulated_ratios(is_bias)
    print(worst)
    assert worst['g'] <= 1.0 and worst['v'] <= 1.0 and worst['w'] <= 1.0, worst
    assert worst['g'] >= 0.2 and worst['v'] >= 0.1 and worst['w'] >= 0.1, worst


@pytest.mark.parametrize('is_bias', [False, True])
def test_bounds_see_a_wrong_bias_correction_and_a_wrong_second_moment(is_bias):
    assert _emulated_ratios(is_bias, wrong='a1')['w'] > 100.0
    assert _emulated_ratios(is_bias, wrong='v')['v'] > 100.0


SHAPES = {}
for _name, _spec in PS.CASES.items():
    SHAPES.setdefault(PS.shape_key(_spec), _name)


@pytest.fixture(scope='module')
def pkg():
    import bayes_sim_ig_amd as B
    B.MDNN.VERBOSE = False
    return B


@pytest.mark.parametrize('name', sorted(SHAPES.values()))
def test_allowed_gradient_error_is_small_against_kernel_mistakes(pkg, name):
    """At the cap M = 16 and the fp32 oracle's own error r, the permitted q = 16 max(r, R_FLOOR) is at most 1/4 of
    the relative change of the fp64 gradient, in every tensor and at every step, under: (a) one minibatch row dropped,
    (b) duplicate ids counted once, (c) the gradient scaled by B / (B - 1), (d) the gradient taken at w_{t-2}."""
    spec = PS.CASES[name]
    ref, state = PS.host_reference(pkg, spec)
    ids, b = PS.case_ids(spec), spec['batch']
    names = list(state)
    states = [state]
    worst = {}
    for t in (1, 2, 3):
        rows = ids[t - 1]
        _, g64 = ref.grad(states[-1], rows, torch.float64)
        _, g32 = ref.grad(states[-1], rows, torch.float32)
        uniq = np.unique(rows)
        assert len(uniq) < b, 'the minibatch has no duplicate id'
        mut = {'a': {k: v * (b - 1.0) / b for k, v in ref.grad(states[-1], rows[:-1])[1].items()},
               'b': {k: v * len(uniq) / b for k, v in ref.grad(states[-1], uniq)[1].items()},
               'c': {k: v * b / (b - 1.0) for k, v in g64.items()}}
        if t >= 2:
            mut['d'] = ref.grad(states[-2], rows)[1]
        for k in names:
            allowed = PS.M_CAP * max(PS.rel_err(g32[k], g64[k]), PS.R_FLOOR)
            for tag, g in mut.items():
                change = PS.rel_err(g[k], g64[k])
                worst[tag] = min(worst.get(tag, np.inf), change / allowed)
                assert allowed <= 0.25 * change, (name, t, k, tag, allowed, change)
        # the next weights: the fp64 step, rounded to the floats a kernel would hold
        flat = np.concatenate([states[0][k].reshape(-1) for k in names]).astype(np.float64)
        gs = []
        for s in states:
            gs.append(np.concatenate([ref.grad(s, ids[len(gs)])[1][k].reshape(-1) for k in names]))
        w_next = PS.adam_replay64(flat, gs, HY)[-1][0].astype(np.float32)
        nxt, o = {}, 0
        for k in names:
            nxt[k] = w_next[o:o + state[k].size].reshape(state[k].shape)
            o += state[k].size
        states.append(nxt)
    print(name, 'least change / allowed error per mutation:', {k: round(v, 1) for k, v in worst.items()})
