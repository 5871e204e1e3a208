"""The core BayesSim class on MI355X — counterpart of the reference's
bayes_sim_ig/bayes_sim.py (class BayesSim: same constructor, constants,
``run_training`` / ``predict`` / ``get_n_trajs_per_batch``).

The reference's file cannot travel with this repo; this orchestrator keeps
its behaviour (summarizer and model picked by name from ``model_cfg``, the
hard-coded chunk schedule of bayes_sim.py:20-25, the multi-trajectory refit
of :148-179) and drives the HIP summarizers and estimators.  ``fit`` adds the
caller-side chunk loop of bayes_sim_main.py:157-167 for pre-recorded pairs.
"""
import os

import numpy as np
import torch

from . import _lib
from . import pdf
from .mdnn import MDNN
from .mdrff import MDRFF
from .summarizer_table import SUMMARIZERS, given as _given
from .summarizers import check_lengths as _check_lengths
from .summarizers import (pad_states_actions, summary_start, summary_waypts,  # noqa: F401
                          summary_corr, summary_corrdiff, summary_signatory,
                          signature_depth, cross_correlation, summary_logsignature,
                          summary_xcorr, summary_kme, summary_sysid)

_MODELS = {'MDNN': MDNN, 'MDRFF': MDRFF}


class BayesSim(object):
    # The reference's protocol constants (bayes_sim.py:20-25), same names and values -- the chunk size a
    # run_training call consumes, how often a chunk is swept, the SGD minibatch, the held-out share:
    NUM_TRAIN_TRAJ_PER_BATCH = 1000  # (theta, trajectory) pairs per run_training call ("chunk")
    NUM_TRAIN_EPOCHS = 10            # sweeps over a chunk
    MINIBATCH_SIZE = 100             # rows per Adam update
    NUM_GRAD_UPDATES = NUM_TRAIN_EPOCHS * NUM_TRAIN_TRAJ_PER_BATCH // MINIBATCH_SIZE   # = 100 updates per chunk
    TEST_FRACTION = 0.2              # last 20 % of a chunk: held out (mdnn.py:206-211)
    FIT_BLOCK_CHUNKS = 32            # (not in the reference) chunks summarised / projected at once by fit()
    # the multi-trajectory refit of predict(): literals in the reference (bayes_sim.py:162,173-174)
    REFIT_SAMPLES = int(1e4)         # samples drawn from the per-trajectory MoGs
    REFIT_MINIBATCH = 100
    REFIT_EPOCHS = 5

    def __init__(self, model_cfg, obs_dim, act_dim, params_dim, params_lows,
                 params_highs, prior, proposal=None, device='cpu'):
        """Arguments as in the reference (bayes_sim.py:27-52).  Optional ``model_cfg`` keys beyond the
        reference's, and values of ``'summarizerFxn'`` that the reference does not have:

        - ``nFeat``: RFF features, default 200 as hard-coded at bayes_sim.py:81.
        - ``sigDepth``: 1..6, the truncation depth of ``summary_signatory`` and ``summary_logsignature``;
          default: the reference's rule, at most 3.
        - ``sigChannels`` (those two summarizers only): the channels of ``[states | actions]`` that make up the
          path after the time channel, in any order -- index ``c < obs_dim`` is a state channel, any other
          action channel ``c - obs_dim``; they are gathered by the kernel, the trajectories are not sliced.
          ``input_dim`` follows from both keys, and a shape whose levels do not fit a workgroup's LDS at
          ``trainTrajLen`` is a NotImplementedError here; include/bsig_signature.h.
        - ``'summarizerFxn': 'summary_logsignature'``: the log-signature of the same path at the Lyndon words,
          ``logsignature_dim`` inputs instead of ``signature_dim``, under the same LDS condition;
          include/bsig_logsignature.h.
        - ``'summarizerFxn': 'summary_xcorr'``: the paper's time-lagged cross-correlation of the state
          differences in time with the actions plus their mean and standard deviation, ``xcorr_dim`` inputs
          from the whole trajectory; include/bsig_xcorr.h.  Its own keys:

          - ``xcorrLags``: an int >= 0, default 0, the largest lag, below the number of feature steps of
            ``trainTrajLen`` states;
          - ``xcorrStateDiff``: a bool, default True; False: the states themselves.
        - ``'summarizerFxn': 'summary_kme'``: the random-feature kernel mean embedding of the transitions
          ``[s_t | a_t | s_(t+1) - s_t]``, ``kmeFeatures`` inputs from every step whatever the task's dimensions
          and length; include/bsig_kme.h.  The per-column scale is made on the device from the first chunk's
          first training trajectories and kept, with the frequencies, in ``bs.embedding.state_dict()``.  Its
          own keys:

          - ``kmeFeatures``: an even int >= 2, default 256;
          - ``kmeScale``: a positive float, default 1.0; times each column's standard deviation times sqrt(d)
            is that column's bandwidth;
          - ``kmeSeed``: an int >= 0, default 0, the frequencies' own generator;
          - ``kmeDiff``: a bool, default True; False: no state differences in the rows;
          - ``kmeTime``: a bool, default False; True: the step's position leads the row.
        - ``'summarizerFxn': 'summary_sysid'``: the ridge least-squares fit of ``s_(t+1) - s_t`` on
          ``[1 | s_t | a_t]`` over the trajectory's own steps and the root mean square of what it leaves,
          ``sysid_dim`` deterministic inputs from the whole trajectory; a shape that does not fit a
          workgroup's LDS at ``trainTrajLen`` is a NotImplementedError here; include/bsig_sysid.h.  Its own
          key:

          - ``sysidRidge``: a positive float, default 1e-3, times the mean diagonal of the Gram matrix; the
            solved system's condition number is at most 1 + (1 + obs_dim + act_dim) / sysidRidge.
        - ``dtype``: 'float32', the default, or 'float64': the estimator's fp64 mode, as ``bs.model.double()``.
        - ``summaryDtype``: 'float32', the default in both modes: the summaries are made in fp32 and a double
          model gets them widened.  'float64', only with ``'dtype': 'float64'``: the summarizers compute in
          double too, so nothing between the trajectories and the posterior is rounded to fp32.
        - ``inputNorm``: a bool, default False.  True: the model is built with ``input_norm=True`` and
          standardises the summaries -- per-column mean and standard deviation of the first chunk's training
          rows, made on the device, kept in ``state_dict`` and applied alike by ``fit``, ``run_training`` and
          ``predict``; constant columns become zero; include/bsig_input_norm.h.  Meant for ``sigDepth`` >= 3,
          whose raw terms reach (trainTrajLen - 1)^k / k!.
        - ``rffSigmaScale``: a positive float, default 1.0, only with ``'modelClass':
          'MDRFF_<kernel>_median'``: that model class sets the RFF bandwidth by the median heuristic --
          ``rffSigmaScale`` times the median pairwise distance of the first chunk's training rows, standardised
          first under ``inputNorm``, made on the device, kept in ``state_dict``; include/bsig_rff_bandwidth.h.

        ``bs.summary_kwargs`` holds the keyword arguments every summarizer call gets from these keys.

        Recorded episodes that end early (the recorder fills the tail with the last state): ``fit`` and
        ``run_training`` take ``traj_lengths``, ``predict`` and the three ``fit_*`` below ``lengths`` -- the valid
        STATES of every trajectory, an int32 / int64 tensor, a numpy integer array or a list -- with
        ``'summary_xcorr'`` and ``'summary_kme'``, whose rows are then those of the trajectories cut at their
        lengths (include/bsig_ragged.h); ValueError with any other summarizer.  Lengths on the host are
        range-checked, lengths on the device are never read back -- one outside the range makes its summary NaN,
        which the deferred finite assert reports -- but for the embedding's scale, which reads back the first
        256 at most, once."""
        self.prior = prior
        self.proposal = proposal
        model_class = model_cfg['modelClass']
        name = model_cfg['summarizerFxn']
        if name not in SUMMARIZERS:
            raise NameError("name '%s' is not defined" % name)   # eval() in the reference
        entry = self._summarizer = SUMMARIZERS[name]
        self.summarizer_name = name
        self.summarizer_fxn = entry.fxn
        sig_depth = model_cfg.get('sigDepth', None)        # owned by nobody: range-checked for every name
        if sig_depth is not None and not 1 <= sig_depth <= _lib.SIGNATURE_MAX_DEPTH:
            raise ValueError("model_cfg['sigDepth'] must be in 1..%d, got %r"
                             % (_lib.SIGNATURE_MAX_DEPTH, sig_depth))
        for other in SUMMARIZERS.values():
            for key, owner in other.keys.items():
                if key not in entry.keys and _given(model_cfg, key):
                    raise ValueError("model_cfg[%r] applies to %r, not to %r" % (key, owner, name))
        # the reference pushes a zero trajectory through the summarizer to get
        # the width (bayes_sim.py:57-60); the width is a closed form
        itemsize = 8 if model_cfg.get('summaryDtype', 'float32') == 'float64' else 4
        traj_summaries_dim, self._summary_kwargs = entry.configure(model_cfg, obs_dim, act_dim, itemsize)
        full_covariance = bool(model_cfg.get('fullCovariance', False))
        kwargs = {'input_dim': traj_summaries_dim, 'output_dim': params_dim,
                  'output_lows': params_lows, 'output_highs': params_highs,
                  'n_gaussians': model_cfg['components'],
                  'hidden_layers': model_cfg['hiddenLayers'],
                  'lr': model_cfg['lr'],
                  'activation': torch.nn.Tanh,
                  'full_covariance': full_covariance,
                  'device': device}
        if model_class.startswith('MDRFF'):      # "MDRFF_<kernel>_<sigma>"
            kernel, sigma = 'RBF', 4.0
            if '_' in model_class:
                parts = model_class.split('_')
                model_class, kernel = parts[0], parts[1]
                if len(parts) > 2:
                    sigma = 'median' if parts[2] == 'median' else float(parts[2])
            kwargs.update({'n_feat': int(model_cfg.get('nFeat', 200)),
                           'sigma': sigma, 'kernel': kernel})
        if 'rffSigmaScale' in model_cfg:
            scale = model_cfg['rffSigmaScale']
            if kwargs.get('sigma') != 'median':
                raise ValueError("model_cfg['rffSigmaScale'] applies to 'modelClass': 'MDRFF_<kernel>_median', "
                                 "not to %r" % (model_cfg['modelClass'],))
            if not isinstance(scale, float) or not (np.isfinite(scale) and scale > 0.0):
                raise ValueError("model_cfg['rffSigmaScale'] must be a positive float, got %r" % (scale,))
            kwargs['sigma_scale'] = scale
        if model_class not in _MODELS:
            raise NameError("name '%s' is not defined" % model_class)
        dtype = model_cfg.get('dtype', 'float32')
        if dtype not in ('float32', 'float64'):
            raise ValueError("model_cfg['dtype'] must be 'float32' or 'float64', got %r" % (dtype,))
        summary_dtype = model_cfg.get('summaryDtype', 'float32')
        if summary_dtype not in ('float32', 'float64'):
            raise ValueError("model_cfg['summaryDtype'] must be 'float32' or 'float64', got %r" % (summary_dtype,))
        if summary_dtype == 'float64' and dtype != 'float64':
            raise ValueError("model_cfg['summaryDtype'] = 'float64' needs model_cfg['dtype'] = 'float64' "
                             "(an fp32 estimator would round the double summaries)")
        self._summary_dtype = torch.float64 if summary_dtype == 'float64' else None
        matmul = model_cfg.get('matmulPrecision', None)
        if matmul is not None and matmul not in ('float32', 'split_bf16'):
            raise ValueError("model_cfg['matmulPrecision'] must be 'float32' or 'split_bf16', got %r" % (matmul,))
        if matmul == 'split_bf16' and dtype == 'float64':
            raise ValueError("model_cfg['matmulPrecision'] = 'split_bf16' applies to an fp32 estimator, "
                             "not to model_cfg['dtype'] = 'float64'")
        input_norm = model_cfg.get('inputNorm', False)
        if not isinstance(input_norm, bool):
            raise ValueError("model_cfg['inputNorm'] must be a bool, got %r" % (input_norm,))
        if input_norm:
            kwargs['input_norm'] = True
        self.model = _MODELS[model_class](**kwargs)
        if matmul is not None:
            self.model.set_matmul_precision(matmul)
        if dtype == 'float64':
            self.model.double()
        # the summarizer's module, where it has one, is built once the model above has made its draws (it has a
        # generator of its own all the same)
        self.embedding = entry.embedding(model_cfg, obs_dim, act_dim, device) if entry.embedding else None

    @property
    def summary_kwargs(self):
        """The keyword arguments every call of the summarizer gets from ``model_cfg`` (its ``configure``'s)."""
        return self._summary_kwargs

    @staticmethod
    def get_n_trajs_per_batch(n_train_trajs, n_train_trajs_done):
        n = BayesSim.NUM_TRAIN_TRAJ_PER_BATCH
        if n_train_trajs_done + n > n_train_trajs:
            n = n_train_trajs - n_train_trajs_done
        return n

    def _ragged_lengths(self, lengths, states):
        """``lengths`` as the summarizer takes them, checked before any GPU call (None stays None); ValueError
        where the summarizer takes none."""
        if lengths is None:
            return None
        if not self._summarizer.ragged:
            raise ValueError("lengths apply to 'summary_xcorr' and 'summary_kme', not to %r"
                             % (self.summarizer_name,))
        diff = self.embedding.diff if self.embedding is not None else self._summary_kwargs.get('state_diff', True)
        return _check_lengths(lengths, int(states.shape[0]), int(states.shape[1]), diff)

    def _summarize(self, states, actions, finite_flag=None, lazy=False, lengths=None):
        entry, kw = self._summarizer, dict(self._summary_kwargs)
        lengths = self._ragged_lengths(lengths, states)
        if lengths is not None:       # (without lengths: no keyword, the call it always was)
            kw['lengths'] = lengths
        # ('summaryDtype': 'float64' -- the summarizers' fp64 kernels; else no keyword: the fp32 path)
        if self._summary_dtype is not None:
            kw['dtype'] = self._summary_dtype
        if entry.check_finite and finite_flag is not None:
            # the isfinite assert of summarizers.py:120, deferred with the chunk's logs
            kw['check_finite'] = finite_flag
        # training never needs the outer product itself: the estimator's first layer forms
        # it from the factor rows (summarizers.CrossCorrFactors)
        if entry.lazy and lazy and self._lazy_summaries():
            kw['lazy'] = True
        args = (states, actions) if entry.embedding is None else (states, actions, self.embedding)
        return self.summarizer_fxn(*args, **kw)

    def _lazy_summaries(self):
        # (a double model takes summary rows only: materialised by the summarizer kernels -- in fp32 and
        # widened, or in double with 'summaryDtype': 'float64')
        # (nor does a model that standardises its inputs: the standardised outer product does not factor)
        return (self.model.rff is None and self.model._flat.is_cuda and not self.model._f64 and
                self.model._inorm is None and os.environ.get('BSIG_NO_FUSED_SUMMARY') != '1')

    def run_training(self, params, traj_states, traj_actions, _defer=False, _finite_flag=None,
                     _summaries=None, _feats=None, _standardized=False, traj_lengths=None):
        """One chunk: summarize, then NUM_GRAD_UPDATES Adam updates of
        MINIBATCH_SIZE (reference bayes_sim.py:91-114).  ``traj_lengths``: the valid states of every
        trajectory ('summary_xcorr' and 'summary_kme'; see the constructor)."""
        if _summaries is None:
            traj_lengths = self._ragged_lengths(traj_lengths, traj_states)
            self._embedding_scale_of_chunk(traj_states, traj_actions, traj_lengths)
        traj_summaries = _summaries if _summaries is not None else \
            self._summarize(traj_states, traj_actions, _finite_flag, lazy=True, lengths=traj_lengths)
        kw = {} if _feats is None else {'_feats': _feats}
        if _standardized:       # fit() has standardised the block these rows come from
            kw['_standardized'] = True
        return self.model.run_training(
            x_data=traj_summaries, y_data=params,
            n_updates=BayesSim.NUM_GRAD_UPDATES,
            batch_size=BayesSim.MINIBATCH_SIZE,
            test_frac=BayesSim.TEST_FRACTION, _defer=_defer, **kw)

    def _require_embedding(self):
        if self.embedding is None:
            raise RuntimeError("this BayesSim was built without 'summarizerFxn': 'summary_kme'")
        return self.embedding

    def fit_embedding_scale(self, states, actions, lengths=None):
        """The per-column scale of ``'summarizerFxn': 'summary_kme'`` from the given trajectories (the first
        256 at most; ``fit`` and ``run_training`` by themselves take the first chunk's first training
        trajectories), frozen from here on.  Synchronises, and asserts that the scale is finite.  ``lengths``:
        from the valid rows only (``KernelMeanEmbedding.fit_scale``: lengths on the device are read back, 1 KB
        at most)."""
        emb = self._require_embedding()
        lengths = self._ragged_lengths(lengths, states)
        if lengths is None:
            emb.fit_scale(states, actions, dtype=self._summary_dtype)
        else:
            emb.fit_scale(states, actions, dtype=self._summary_dtype, lengths=lengths)
        return self._keep_if_finite(emb, (emb.inv_std,), 'non-finite value in the trajectories')

    def _keep_if_finite(self, stat, values, message):
        """The end of every ``fit_*`` below: one read-back of whether the ``values`` just made for the frozen
        statistic ``stat`` are all finite; if not, ``stat`` is back to "not there yet" and ``message`` is an
        AssertionError."""
        finite = torch.isfinite(values[0]).all()
        for value in values[1:]:
            finite = finite & torch.isfinite(value).all()
        if not bool(finite.item()):
            stat.reset()
            raise AssertionError(message)
        return self

    @staticmethod
    def _first_training_rows(n, done=0):
        """How many rows of the chunk that starts at pair ``done`` of ``n`` are training rows (the chunk's last
        rows are held out): what a statistic that does not exist yet is made from, on every path."""
        return _lib.split_rows(BayesSim.get_n_trajs_per_batch(n, done), BayesSim.TEST_FRACTION)[0]

    def _embedding_scale_of_chunk(self, states, actions, lengths=None):
        """The scale, where it does not exist yet, from the trajectories both paths of ``fit`` and
        ``run_training`` use: the first ``min(n_train, 256)`` of the chunk ``states`` starts with.  Nothing is
        read back: a non-finite trajectory among them makes every summary non-finite, which the summaries'
        finite flag reports.  With ``lengths`` (checked already): from those trajectories' valid rows; lengths
        on the device are read back here, the first 256 at most, once per embedding."""
        emb = self.embedding
        if emb is None or emb.ready:
            return
        emb.refuse_data_parallel(self.model._dp)
        n_train = self._first_training_rows(int(states.shape[0]))
        if lengths is None:
            emb.fit_scale(states[:n_train], actions[:n_train], dtype=self._summary_dtype)
        else:
            emb.fit_scale(states[:n_train], actions[:n_train], dtype=self._summary_dtype,
                          lengths=lengths[:n_train])

    def fit_input_norm(self, states, actions, lengths=None):
        """The input statistics of a model built with ``'inputNorm': True`` from the summaries of ALL the
        given trajectories (``fit`` by itself takes the first chunk's training rows), frozen from here on.
        Synchronises, and asserts that the statistics are finite."""
        norm = self.model._require_inorm()
        self.model.fit_input_norm(self._summarize(states, actions, lengths=lengths))
        return self._keep_if_finite(norm, (norm.mean, norm.inv_std), 'non-finite value in the trajectory summaries')

    def fit_rff_bandwidth(self, states, actions, lengths=None):
        """The counterpart of ``fit_input_norm`` for the bandwidth of an ``'MDRFF_<kernel>_median'`` model: from
        the summaries of the given trajectories (the first 1024 at most; ``fit`` by itself takes the first
        chunk's training rows), standardised first under ``inputNorm``, frozen from here on.  Synchronises, and
        asserts that the bandwidth is finite."""
        bw = self.model._require_rffbw()
        self.model.fit_rff_bandwidth(self._summarize(states, actions, lengths=lengths))
        return self._keep_if_finite(bw, (bw.sigma,), 'non-finite value in the trajectory summaries')

    def _standardize_block(self, summ, n_train):
        """fit()'s block path for a model with input_norm: the statistics, where they do not exist yet, from
        the rows the chunk loop would have used -- the ``n_train`` training rows of the first chunk -- then the
        block standardised in place, once, in the model's precision.  Nothing is read back."""
        model = self.model
        summ, ld, prec = model._input_rows(summ, model._prec.dtype)
        if not model.input_norm_ready:
            model._stats_of(summ, ld, n_train, prec)
        return model.normalize_inputs(summ, out=summ)

    FIT_BLOCK_BYTES = 4 << 30        # (not in the reference) bound on a block's summaries in fit()

    def fit(self, params, traj_states, traj_actions, traj_lengths=None):
        """The caller-side loop of bayes_sim_main.py:157-167 over
        pre-recorded pairs: consecutive chunks of at most
        NUM_TRAIN_TRAJ_PER_BATCH pairs, ``run_training`` on each.
        Returns the list of per-chunk log dicts.  ``traj_lengths``: the valid states of every trajectory
        ('summary_xcorr' and 'summary_kme'; see the constructor), sliced with the trajectories."""
        traj_lengths = self._ragged_lengths(traj_lengths, traj_states)
        # the chunks' logs are read after the last chunk is enqueued: if a persistent launch turns out not
        # to have had the GPU to itself, the whole loop is repeated from here (MDNN._retrying)
        return self.model._retrying(lambda: self._fit_once(params, traj_states, traj_actions, traj_lengths))

    def _check_equal_counts(self, n):
        """One all-reduce per update: every rank of a data-parallel group must run the same chunk
        schedule, or the rank with an extra chunk waits for its peers forever."""
        if self.model._dp is not None:
            counts = self.model._dp.gather_counts(n, device=self.model._flat.device)
            if len(set(counts)) != 1:
                raise ValueError('data-parallel fit needs the same number of pairs on every rank '
                                 '(got %s); see dp.equal_shards' % (counts,))

    def _block_rows(self):
        """Pairs per block of fit(): the summaries (and an MDRFF's RFF features, rff.py:128-132) are pure
        functions of the row, so both are computed for a block of chunks at once -- one summarizer launch
        over up to 32000 trajectories (and one large MFMA GEMM) instead of one small one per chunk."""
        summary_bytes = 8 if self._summary_dtype == torch.float64 else 4
        row_bytes = summary_bytes * self.model.input_dim + \
            4 * (self.model.rff.n_feat if self.model.rff is not None else 0)
        chunks = max(min(BayesSim.FIT_BLOCK_CHUNKS,
                         BayesSim.FIT_BLOCK_BYTES // (row_bytes * BayesSim.NUM_TRAIN_TRAJ_PER_BATCH)), 1)
        return chunks * BayesSim.NUM_TRAIN_TRAJ_PER_BATCH

    def _block_launch_sizes(self, n, lo, hi):
        """The chunks of pairs [lo, hi) of ``n`` that one launch can take (a chunk without a held-out row
        runs on its own)."""
        sizes, at = [], lo
        while at < hi:
            sizes.append(BayesSim.get_n_trajs_per_batch(n, at))
            at += sizes[-1]
        return sizes[:self.model.block_prefix(sizes, BayesSim.TEST_FRACTION)]

    def _fit_once(self, params, traj_states, traj_actions, traj_lengths=None):
        """Block by block: the block's summaries and features when ``done`` leaves the block before; the
        block's chunks in ONE launch of the persistent update kernel where the model's plan can; else chunk
        by chunk.  The logs (and the isfinite asserts) are read back after the last chunk is enqueued: one
        host synchronisation for the whole fit.  A model with input_norm: each block is standardised once,
        before an MDRFF's features are projected from it, and its chunks are handed over as standardised.
        An ``'MDRFF_<kernel>_median'`` model: the bandwidth is made from the first block, after that and
        before the projection."""
        model, n, done, pending = self.model, params.shape[0], 0, []
        model._check_statistics_dp()
        self._embedding_scale_of_chunk(traj_states, traj_actions, traj_lengths)
        if traj_lengths is not None and torch.is_tensor(traj_states) and traj_states.is_cuda:
            # (the scale above took them where they were: lengths on the host are not read back)
            traj_lengths = traj_lengths.to(traj_states.device)      # once, not once per chunk
        cut = lambda a, b: None if traj_lengths is None else traj_lengths[a:b]      # noqa: E731
        self._check_equal_counts(n)
        on_gpu = torch.is_tensor(traj_states) and traj_states.is_cuda
        flag = torch.zeros(1, dtype=torch.int32, device=traj_states.device) if on_gpu else None
        block = self._block_rows() if on_gpu and os.environ.get('BSIG_NO_FIT_PREPROJECT') != '1' else 0
        lo = hi = 0
        summ = feats = None
        while done < n:
            if block and done >= hi:
                lo, hi = done, min(n, done + block)
                summ = self._summarize(traj_states[lo:hi], traj_actions[lo:hi], flag, lazy=True, lengths=cut(lo, hi))
                if model._inorm is not None:
                    summ = self._standardize_block(summ, self._first_training_rows(n, lo))
                if model._rffbw is not None and not model.rff_bandwidth_ready:
                    # the bandwidth of the rows the chunk loop would have used: the first chunk's training
                    # rows, as the projection sees them; nothing is read back
                    model._bandwidth_of_rows(summ[:self._first_training_rows(n, lo)])
                # (a double MDRFF projects in double inside each call: chunk by chunk, no block launch)
                feats = model.rff.to_features(summ) if model.rff is not None and not model._f64 else None
                sizes = self._block_launch_sizes(n, lo, hi) if feats is not None and model._dp is None else []
                rows = sum(sizes)
                logs = model.run_training_block(
                    feats[:rows], params[lo:lo + rows], sizes, BayesSim.NUM_GRAD_UPDATES,
                    BayesSim.MINIBATCH_SIZE, BayesSim.TEST_FRACTION) if sizes else None
                if logs is not None:
                    pending.extend(logs)
                    done += rows
                    continue
            m = BayesSim.get_n_trajs_per_batch(n, done)
            if block:
                pending.append(self.run_training(
                    params[done:done + m], None, None, _defer=True,
                    _summaries=summ[done - lo:done - lo + m], _standardized=model._inorm is not None,
                    _feats=None if feats is None else feats[done - lo:done - lo + m]))
            else:
                pending.append(self.run_training(params[done:done + m],
                                                 traj_states[done:done + m],
                                                 traj_actions[done:done + m], _defer=True,
                                                 _finite_flag=flag, traj_lengths=cut(done, done + m)))
            done += m
        logs = [p.result() for p in pending]
        assert flag is None or int(flag.item()) == 0   # summarizers.py:120
        return logs

    def predict(self, states, actions, threshold=0.005, lengths=None):
        """Posterior for the given real trajectories (the contract of reference bayes_sim.py:116-179):
        ONE trajectory -> the model's mixture for it (divided by the proposal when there is one);
        SEVERAL -> REFIT_SAMPLES draws from their mixtures, refitted by a fresh unconditional MDNN
        (input: a constant) whose single mixture is returned.  ``lengths``: the valid states of every
        trajectory ('summary_xcorr' and 'summary_kme'; see the constructor)."""
        summaries = self._summarize(states, actions, lengths=lengths)
        mixtures = [self._correct_for_proposal(m, threshold) for m in self.model.predict_MoGs(summaries)]
        return mixtures[0] if len(mixtures) == 1 else self._refit(mixtures)

    def _correct_for_proposal(self, mog, threshold):
        """bayes_sim.py:135-145: prune, then posterior = mixture x prior / proposal (a uniform prior drops out)."""
        if self.proposal is None:
            return mog
        mog.prune_negligible_components(threshold=threshold)
        if isinstance(self.prior, pdf.Uniform):
            return mog / self.proposal
        if isinstance(self.prior, pdf.Gaussian):
            return (mog * self.prior) / self.proposal
        raise NotImplementedError

    def _refit(self, mixtures):
        """bayes_sim.py:149-179: equal shares of REFIT_SAMPLES from every trajectory's mixture, REFIT_EPOCHS
        sweeps of minibatch REFIT_MINIBATCH through the fit engine (the estimator's own hyper-parameters,
        a [128, 128] trunk on a constant input), the fitted model's mixture at that input."""
        src = self.model
        refit = MDNN(input_dim=1, output_dim=src.output_dim,
                     output_lows=src.output_lows.detach().cpu().numpy(),
                     output_highs=src.output_highs.detach().cpu().numpy(),
                     n_gaussians=src.n_gaussians, hidden_layers=(128, 128), lr=src.lr,
                     activation=src.activation, full_covariance=src.L_size > 0, device=src.device)
        if src._f64:
            refit.double()
        share = int(BayesSim.REFIT_SAMPLES / len(mixtures))
        draws = torch.from_numpy(np.concatenate([m.gen(n_samples=share) for m in mixtures], axis=0))
        draws = draws.to(src._dtype).to(src.device)
        if MDNN.VERBOSE:
            print(f'Fitting posterior from {len(mixtures):d} mogs')
        const_in = torch.zeros(draws.shape[0], 1, dtype=src._dtype, device=draws.device)
        refit.run_training(const_in, draws,
                           BayesSim.REFIT_EPOCHS * BayesSim.REFIT_SAMPLES // BayesSim.REFIT_MINIBATCH,
                           BayesSim.REFIT_MINIBATCH)
        fitted = refit.predict_MoGs(const_in[0:1, :])
        assert len(fitted) == 1
        return fitted[0]
