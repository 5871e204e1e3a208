"""CPU-side checks of what the three frozen statistics share (bayes_sim_ig_amd/frozen.py): ``ready`` follows
``count`` through ``load_state_dict``, the buffers keep their dtypes, ``require_ready`` names the remedy, and each
subclass's "the value changed" hook fires where it did before the base existed.  One list for all three: where
tests/test_input_norm_host.py, tests/test_rff_bandwidth_host.py or tests/test_kme_host.py assert an item for one of
them through its model, it is asserted here on the module itself."""
import numpy as np
import pytest
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd.frozen import FrozenStatistic
from bayes_sim_ig_amd.mdnn import InputNorm, RffBandwidth


def _statistics():
    return {'fit_input_norm': InputNorm(5, 'cpu'), 'fit_rff_bandwidth': RffBandwidth(1.0, 'cpu'),
            'fit_scale': B.KernelMeanEmbedding(3, 1, n_feat=16)}


def test_the_three_derive_from_one_base_and_not_from_each_other():
    stats = list(_statistics().values())
    assert all(isinstance(s, FrozenStatistic) for s in stats)
    assert not isinstance(stats[1], InputNorm)
    assert [list(s.state_dict()) for s in stats] == [['mean', 'inv_std', 'count'], ['sigma', 'count'],
                                                     ['freqs', 'inv_std', 'count']]


@pytest.mark.parametrize('remedy', ['fit_input_norm', 'fit_rff_bandwidth', 'fit_scale'])
def test_ready_follows_count_and_the_dtypes_stay(remedy):
    stat, twin = _statistics()[remedy], _statistics()[remedy]
    assert stat.ready is False and int(stat.count) == 0
    with pytest.raises(RuntimeError, match=remedy):
        stat.require_ready()
    dtypes = {k: v.dtype for k, v in stat.state_dict().items()}
    assert dtypes['count'] == torch.int64
    stat.double().float()
    assert {k: v.dtype for k, v in stat.state_dict().items()} == dtypes
    # a state made from no rows leaves the statistic without a value
    twin.load_state_dict(stat.state_dict())
    assert twin.ready is False
    with pytest.raises(RuntimeError, match=remedy):
        twin.require_ready()
    # ... and one made from some gives it
    state = stat.state_dict()
    state['count'] = torch.tensor(7)
    twin.load_state_dict(state)
    assert twin.ready is True and int(twin.count) == 7 and twin.require_ready() is twin
    # a state without the count decides nothing
    del state['count']
    twin.load_state_dict(state, strict=False)
    assert twin.ready is True
    # the refusal under data parallel: only while the value does not exist
    twin.refuse_data_parallel(object())
    stat.refuse_data_parallel(None)
    with pytest.raises(ValueError, match='data-parallel.*%s' % ('fit_embedding_scale' if remedy == 'fit_scale'
                                                               else remedy)):
        stat.refuse_data_parallel(object())
    twin.reset()
    assert twin.ready is False and int(twin.count) == 0


def test_the_bandwidth_counts_every_value_it_is_given():
    bw = _statistics()['fit_rff_bandwidth']
    assert bw.version == 0
    bw.load_state_dict(bw.state_dict())                  # every load, whatever it holds
    assert bw.version == 1
    bw.made_from(3)
    assert bw.version == 2 and bw.ready and int(bw.count) == 3
    bw.double().to('cpu')                                # a move is not a new value
    assert bw.version == 2
    bw.reset()
    assert bw.version == 2 and not bw.ready


def test_the_embedding_drops_its_coefficients_with_the_value_and_with_a_move():
    emb = _statistics()['fit_scale']
    stale = {4: torch.zeros(8, 8)}
    for change in (lambda: emb.load_state_dict(emb.state_dict()), lambda: emb.to('cpu'), lambda: emb.double(),
                   lambda: emb.set_scale(np.ones(7)), lambda: emb.made_from(2)):
        emb._coeff = dict(stale)
        change()
        assert emb._coeff == {}
