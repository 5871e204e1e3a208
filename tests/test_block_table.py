"""Host logic of the block launch (several chunks of a fit in one launch of the persistent update kernel):
the chunk table handed to bsig_fit_run_block against a plain restatement, which chunks of a block one launch
may take, the engine's resolved "several chunks per launch" answer, and the first level a time-out gives
up.  No GPU."""
import ctypes as C
import warnings

import numpy as np
import pytest

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib


def _restated(sizes, seeds, n_updates, batch, test_frac):
    """Chunk after chunk, the way the per-chunk calls lay a chunk out (mdnn.py:206-211, :219-222, :235)."""
    out, row0, upd, ev = [], 0, 0, 0
    for n_tot, seed in zip(sizes, seeds):
        n_train = max(int(n_tot * (1.0 - test_frac)), 1)
        every = max(n_updates // 5, 1)
        n_evals = sum(1 for it in range(n_updates) if it % every == 0 or it + 1 == n_updates)
        out.append(dict(row0=row0, n_train=n_train, n_test=n_tot - n_train, ids_off=upd * batch, seed=seed,
                        rng_ctr0=1, n_updates=n_updates, eval_every=every, train_slot=upd, test_slot=ev,
                        upd_base=upd, eval_base=ev))
        row0, upd, ev = row0 + n_tot, upd + n_updates, ev + n_evals
    return out


@pytest.mark.parametrize('sizes,n_updates,batch', [([1000] * 32, 100, 100), ([1000, 1000, 1000, 400], 100, 100),
                                                   ([1000, 7], 100, 100), ([40] * 32, 7, 16), ([5], 1, 3)])
def test_chunk_table_is_the_per_chunk_layout(sizes, n_updates, batch):
    assert _lib.FIT_CHUNK.itemsize == 64
    seeds = [(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 62) for i in range(len(sizes))]
    table = _lib.fit_chunk_table(sizes, seeds, n_updates, batch, 0.2)
    want = _restated(sizes, seeds, n_updates, batch, 0.2)
    assert len(table) == len(want)
    for row, w in zip(table, want):
        for name, v in w.items():
            assert int(row[name]) == v, name
    # rows, ids and log slots of consecutive chunks neither overlap nor leave gaps
    for a, b in zip(table[:-1], table[1:]):
        assert a['row0'] + a['n_train'] + a['n_test'] == b['row0']
        assert a['ids_off'] + n_updates * batch == b['ids_off']
        assert a['train_slot'] + n_updates == b['train_slot'] and a['test_slot'] < b['test_slot']
    assert table.view(np.int32).shape == (16 * len(sizes),)


def test_block_prefix_stops_at_a_chunk_without_held_out_rows():
    f = B.MDNN.block_prefix
    assert f([1000, 1000, 400], 0.2) == 3
    assert f([1000, 2], 0.2) == 2            # 1 + 1
    assert f([1000, 1], 0.2) == 1            # the one-pair remainder evaluates nothing: on its own
    assert f([1], 0.2) == 0 and f([], 0.2) == 0


def test_engine_answer_for_several_chunks_per_launch():
    lib = _lib.load()
    assert lib.bsig_debug_block_launch(1, 1, 0) == 1      # linear heads, evaluations inside the launch
    assert lib.bsig_debug_block_launch(1, 1, 1) == 0      # BSIG_FIT_CHUNK_PER_LAUNCH=1
    assert lib.bsig_debug_block_launch(1, 0, 0) == 0      # evaluations between the launches
    assert lib.bsig_debug_block_launch(2, 1, 0) == 0      # the MDNN engines
    assert lib.bsig_debug_block_launch(0, 1, 0) == 0      # per-phase kernels
    assert lib.bsig_fit_block_chunks(None, 800) == 0


class _FakeModel:
    _give_up_a_level = B.MDNN._give_up_a_level

    def __init__(self, launches):
        self._dp, self.disabled, self._block_launches = None, 0, launches

    def _disable_persistent(self):
        self.disabled += 1


def test_a_block_launch_time_out_first_costs_the_block_launch():
    m = _FakeModel(launches=3)
    with pytest.warns(RuntimeWarning, match='one launch per chunk'):
        m._give_up_a_level(0, 2)
    assert m._no_block_launch is True and m.disabled == 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m._give_up_a_level(0, 3)             # no block launch since: the persistent kernels go
    assert m.disabled == 1
