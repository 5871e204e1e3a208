"""The precision seam (_lib.F32 / _lib.F64, _lib.as_rows, MDNN._prec): the one place where "fp32 or fp64" is
decided.  Both precisions resolve every shared operation to the right symbol of the library, the two
prototypes of an operation differ by the inserted hyper-parameter pointer alone, an fp64 plan's capabilities
are answered without the library, and a plan is destroyed by the precision that created it.  Host only: a
recording fake stands in for the library wherever a call would need a plan or a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib

P = _lib.Precision
HYPER = C.POINTER(_lib.F64Hyper)
QUERY_ARGS = {'is_persistent': (), 'accepts_factor_rows': (4, 1), 'evaluates_from_factors': (4, 1, 0),
              'takes_features': (100,), 'block_chunks': (100,)}


class FakeLib:
    """Records every call.  What building and casting a model needs (the parameter layout) is forwarded to
    the library; everything else is answered here, nothing real being behind the arguments of these tests: a
    create makes up a handle, a capability query says 7, any other call 0."""
    FORWARD = ('bsig_last_error', 'bsig_mdn_param_count', 'bsig_mdn_param_offsets')

    def __init__(self):
        self.real, self.calls = _lib.load(), []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in self.FORWARD:
                return getattr(self.real, name)(*args)
            if 'create' in name:
                args[-1]._obj.value = 0x1000 + len(self.calls)
                return 0
            return 7 if name in ['bsig_fit_' + q for q in QUERY_ARGS] else 0
        return call

    def names(self, part=''):
        return [n for n, _ in self.calls if part in n]


@pytest.fixture
def fake(monkeypatch):
    """The fake in place of the library, and fresh precision objects that resolve against it."""
    lib = FakeLib()
    monkeypatch.setattr(_lib, '_lib', lib)
    monkeypatch.setattr(_lib, 'F32', P(torch.float32))
    monkeypatch.setattr(_lib, 'F64', P(torch.float64))
    return lib


def _model():
    torch.manual_seed(0)
    return B.MDNN(input_dim=40, output_dim=3, output_lows=np.array([0.1, 0.2, 0.3]),
                  output_highs=np.array([1.0, 2.0, 3.0]), n_gaussians=4, full_covariance=True,
                  hidden_layers=(24, 24), activation=torch.nn.Tanh, lr=1e-3)


def test_attributes():
    f32, f64 = _lib.F32, _lib.F64
    assert (f32.dtype, f32.np_dtype, f32.itemsize, f32.Buffers, f32.state_words) == \
        (torch.float32, np.float32, 4, _lib.FitBuffers, 16)
    assert (f64.dtype, f64.np_dtype, f64.itemsize, f64.Buffers, f64.state_words) == \
        (torch.float64, np.float64, 8, _lib.Fit64Buffers, 32)
    m = _model()
    assert m._prec is _lib.F32 and m.double()._prec is _lib.F64 and m.float()._prec is _lib.F32
    with pytest.raises(AttributeError):
        f32.no_such_entry_point


@pytest.mark.parametrize('op', sorted(P.OPS))
def test_both_precisions_resolve_to_the_library_and_differ_by_the_hyper_alone(op):
    lib = _lib.load()
    n32, n64 = _lib.F32.symbol(op), _lib.F64.symbol(op)
    assert n64 == n32 + '_f64' and n32 == 'bsig_' + n32[5:]
    res32, args32 = _lib.PROTOS[n32]
    res64, args64 = _lib.PROTOS[n64]
    assert n32 not in _lib._PROTOS_F64 and n64 not in _lib._PROTOS       # (and each in its own header, where
    assert (n32 in _lib._PROTOS) == (n64 in _lib._PROTOS_F64)            # the base headers declare the pair)
    widened = [_lib.f64 if a is _lib.f32 else a for a in args32]      # (a float scalar is a double there)
    want = widened[:1] + [HYPER] + widened[1:] if op in P.HYPER_OPS else widened
    assert res64 is res32 and args64 == want
    for name, (res, args) in ((n32, (res32, args32)), (n64, (res64, args64))):
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_plan_lifecycle_symbols():
    lib = _lib.load()
    for op in P.FIT_OPS:
        n32, n64 = _lib.F32.symbol(op), _lib.F64.symbol(op)
        assert n32 in _lib._PROTOS and n64 in _lib._PROTOS_F64 and hasattr(lib, n32) and hasattr(lib, n64)
        assert n64 == 'bsig_fit64_' + op[4:]
    assert _lib.F32.symbol('fit_create') == 'bsig_fit_create_ex'
    for op in ('fit_destroy', 'fit_workspace_bytes', 'fit_begin', 'fit_run'):
        assert _lib._PROTOS['bsig_' + op] == _lib._PROTOS_F64['bsig_fit64_' + op[4:]]
    for prec in (_lib.F32, _lib.F64):
        assert _lib.__dict__['_PROTOS_F64' if prec.itemsize == 8 else '_PROTOS'][prec.symbol('fit_bind')][1][1] \
            == C.POINTER(prec.Buffers)


@pytest.mark.parametrize('op', sorted(P.OPS))
def test_every_operation_reaches_its_symbol_with_or_without_the_hyper(fake, op):
    n_args = len(_lib.PROTOS[_lib.F64.symbol(op)][1])      # the uniform signature is the fp64 one
    args = tuple('arg%d' % i for i in range(n_args))
    getattr(_lib.F32, op)(*args)
    getattr(_lib.F64, op)(*args)
    reaches_f32 = args[:1] + args[2:] if op in P.HYPER_OPS else args
    assert fake.calls == [(_lib.F32.symbol(op), reaches_f32), (_lib.F64.symbol(op), args)]


def test_head_outputs_argument_order(fake):
    rest = ('out', 9, 5, 'noise', 11, 0, 'w', 'mu', 'l_d', 'low', 'flag', 'ws', 64, 'stream')
    _lib.F32.head_outputs('dims', 'hyper', *rest)
    _lib.F64.head_outputs('dims', 'hyper', *rest)
    assert fake.calls == [('bsig_mdn_head_outputs', ('dims',) + rest),
                          ('bsig_mdn_head_outputs_f64', ('dims', 'hyper') + rest)]
    # resolved once: afterwards a plain attribute of the instance
    assert 'head_outputs' in vars(_lib.F32) and 'head_outputs' in vars(_lib.F64)


def test_fp64_capabilities_are_answered_without_the_library(fake):
    plan = C.c_void_p(0x64)
    for q, args in QUERY_ARGS.items():
        assert getattr(_lib.F64, q)(plan, *args) == 0
    assert _lib.F64.fit_set_features(plan, None, 0, 0, None) == _lib.BSIG_EUNSUPPORTED
    assert fake.calls == []
    for q, args in QUERY_ARGS.items():
        assert getattr(_lib.F32, q)(plan, *args) == 7
    assert fake.calls == [('bsig_fit_' + q, (plan,) + args) for q, args in QUERY_ARGS.items()]


def test_plan_lifecycle_calls(fake):
    for prec, stem in ((_lib.F32, 'bsig_fit_'), (_lib.F64, 'bsig_fit64_')):
        del fake.calls[:]
        plan = prec.fit_create('cfg', 'hyper', 10, 48, 12, 5, 0)
        assert plan.value
        create = fake.calls[0]
        if prec is _lib.F32:
            assert create[0] == 'bsig_fit_create_ex' and create[1][:-1] == ('cfg', 10, 48, 12, 5, 0)
        else:
            assert create[0] == 'bsig_fit64_create' and create[1][:-1] == ('cfg', 'hyper', 10, 48, 12, 5)
        prec.fit_workspace_bytes(plan), prec.fit_bind(plan, 'fb', 1), prec.fit_begin(plan, 3, 10, 'st')
        prec.fit_run(plan, 5, 'st'), prec.fit_pack_logs(plan, 5, 2, 'out', 'st'), prec.fit_destroy(plan)
        pack = (plan, 5, 'out', 'st') if prec is _lib.F32 else (plan, 5, 2, 'out', 'st')
        assert fake.calls[1:] == [(stem + 'workspace_bytes', (plan,)), (stem + 'bind', (plan, 'fb', 1)),
                                  (stem + 'begin', (plan, 3, 10, 'st')), (stem + 'run', (plan, 5, 'st')),
                                  (stem + 'pack_logs', pack), (stem + 'destroy', (plan,))]
    # an fp64 plan is per-phase launches by itself; it has no other option
    _lib.F64.fit_create('cfg', 'hyper', 10, 48, 12, 5, _lib.PLAN_NO_PERSISTENT)
    with pytest.raises(NotImplementedError):
        _lib.F64.fit_create('cfg', 'hyper', 10, 48, 12, 5, 2)


def test_a_failing_entry_point_raises(fake, monkeypatch):
    monkeypatch.setattr(FakeLib, 'bsig_copy_rows_f64', lambda self, *a: _lib.BSIG_EUNSUPPORTED, raising=False)
    with pytest.raises(NotImplementedError):
        _lib.F64.copy_rows(None, 0, None, None, 0, 0, 0, None)


def test_a_plan_is_destroyed_by_the_precision_that_created_it(fake):
    m = _model()
    cfg = m._cfg()
    m._ensure_plan(cfg, 10, 48, 12, 5)
    first = m._plan
    assert first.value and m._plan_prec is _lib.F32 and fake.names('bsig_fit') == ['bsig_fit_create_ex']
    m._ensure_plan(cfg, 10, 48, 12, 5)                     # same key: same plan
    assert m._plan is first and fake.names('bsig_fit') == ['bsig_fit_create_ex']
    m._bufs['kept'] = 1
    m._ensure_plan(cfg, 10, 72, 18, 5)                     # grown: a new plan, the call buffers stay
    assert fake.names('bsig_fit') == ['bsig_fit_create_ex', 'bsig_fit_destroy', 'bsig_fit_create_ex']
    assert fake.calls[-2][1][0] is first and m._bufs['kept'] == 1
    assert (m._bufs['cap_train'], m._bufs['cap_test']) == (72, 18)
    second = m._plan
    del fake.calls[:]
    m.double()
    assert fake.names('bsig_fit') == ['bsig_fit_destroy']          # once, and never bsig_fit64_destroy
    assert dict(fake.calls)['bsig_fit_destroy'][0] is second
    assert m._plan is None and m._plan_prec is None and m._bufs == {}
    del fake.calls[:]
    m._no_persistent = True          # given up in fp32 earlier: nothing an fp64 plan has to be told
    m._ensure_plan(m._cfg(), 10, 48, 12, 5)
    assert fake.names('bsig_fit') == ['bsig_fit64_create'] and m._plan_prec is _lib.F64
    hyper = fake.calls[-1][1][1]._obj
    assert isinstance(hyper, _lib.F64Hyper) and hyper.lr == 1e-3
    assert not m._may_time_out()
    third = m._plan
    del fake.calls[:]
    m.float()
    assert fake.names('bsig_fit') == ['bsig_fit64_destroy']        # and the reverse going back
    assert dict(fake.calls)['bsig_fit64_destroy'][0] is third and m._plan is None


class Rows:
    """Stands in for a tensor on its way through as_rows: records every conversion and move."""

    def __init__(self, dtype, device, log, dims=2):
        self.dtype, self.device, self.log, self.dims = dtype, torch.device(device), log, dims
        self.shape = (3, 2, 1)[:dims]

    def to(self, what):
        self.log.append(what)
        if isinstance(what, torch.dtype):
            return Rows(what, self.device, self.log, self.dims)
        return Rows(self.dtype, what, self.log, self.dims)

    is_cuda = property(lambda self: self.device.type == 'cuda')

    def dim(self):
        return self.dims

    def stride(self, i):
        return (2, 1)[i]


def test_as_rows_moves_the_smaller_form():
    log = []
    t, ld = _lib.as_rows(Rows(torch.float64, 'cpu', log), 'cuda:0')
    assert log == [torch.float32, 'cuda:0'] and t.dtype == torch.float32 and ld == 2     # narrowed, then moved
    del log[:]
    t, ld = _lib.as_rows(Rows(torch.float32, 'cpu', log), 'cuda:0', torch.float64)
    assert log == ['cuda:0', torch.float64] and t.dtype == torch.float64                  # moved, then widened
    del log[:]
    _lib.as_rows(Rows(torch.float64, 'cuda:0', log), 'cuda:0', torch.float64)
    assert log == []
    assert _lib.as_f32_rows is _lib.as_rows and not hasattr(_lib, 'as_f64_rows')


def test_as_rows_errors():
    with pytest.raises(RuntimeError, match='expected a GPU tensor'):
        _lib.as_rows(torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='expected a GPU tensor'):
        _lib.as_rows(torch.zeros(3, 2), None, torch.float64)
    log = []
    with pytest.raises(RuntimeError, match='expected a GPU tensor'):      # narrowed before any move is tried
        _lib.as_rows(Rows(torch.float64, 'cpu', log))
    assert log == [torch.float32]
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(AssertionError, match='2-D'):
            _lib.as_rows(Rows(dtype, 'cuda:0', [], dims=3), 'cuda:0', dtype)
