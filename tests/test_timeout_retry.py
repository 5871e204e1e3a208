"""Host logic of the retry after a persistent launch's time-out (MDNN._retrying, behind MDNN.run_training and
BayesSim.fit): the work is repeated from the snapshot, one level further down after each of the first two
time-outs; a third one propagates; where no persistent kernel can run, nothing is saved or repeated.  Pure
Python, no GPU."""
import pytest

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd.mdnn import PersistentTimeout


class _FakeModel:
    _retrying = B.MDNN._retrying
    _give_up_a_level = B.MDNN._give_up_a_level

    def __init__(self, may_time_out=True):
        self._dp, self._block_launches, self._no_block_launch = None, 0, False
        self.may_time_out, self.snapshots, self.restored, self.disabled = may_time_out, 0, [], 0

    def _may_time_out(self):
        return self.may_time_out

    def _snapshot(self):
        self.snapshots += 1
        return 'snapshot %d' % self.snapshots

    def _restore(self, snap):
        self.restored.append(snap)

    def _disable_persistent(self):
        self.disabled += 1


def _work(model, time_outs):
    """A call that launches a block and then times out, ``time_outs`` times; after that it returns its number."""
    calls = []

    def fn():
        calls.append(len(calls) + 1)
        if len(calls) <= time_outs:
            if not model._no_block_launch:
                model._block_launches += 1
            raise PersistentTimeout('call %d' % len(calls))
        return 'result of call %d' % len(calls)
    return fn, calls


@pytest.mark.filterwarnings('ignore::RuntimeWarning')
def test_two_time_outs_cost_two_levels_and_the_third_call_answers():
    m = _FakeModel()
    fn, calls = _work(m, time_outs=2)
    assert m._retrying(fn) == 'result of call 3'
    assert calls == [1, 2, 3]
    assert m.snapshots == 1 and m.restored == ['snapshot 1', 'snapshot 1']
    # the first time-out followed a block launch: the block launch went; the second: the persistent kernels
    assert m._no_block_launch is True and m._block_launches == 1 and m.disabled == 1


@pytest.mark.filterwarnings('ignore::RuntimeWarning')
def test_the_third_time_out_propagates():
    m = _FakeModel()
    fn, calls = _work(m, time_outs=3)
    with pytest.raises(PersistentTimeout, match='call 3'):
        m._retrying(fn)
    assert calls == [1, 2, 3] and m.restored == ['snapshot 1'] * 2
    assert m._no_block_launch is True and m.disabled == 1      # no level is given up for the last one


def test_a_model_that_cannot_time_out_saves_and_repeats_nothing():
    m = _FakeModel(may_time_out=False)
    fn, calls = _work(m, time_outs=0)
    assert m._retrying(fn) == 'result of call 1'
    fn, calls = _work(m, time_outs=1)
    with pytest.raises(PersistentTimeout, match='call 1'):
        m._retrying(fn)
    assert calls == [1] and m.snapshots == 0 and m.restored == [] and m.disabled == 0
