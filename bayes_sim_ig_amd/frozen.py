"""What the opt-in statistics of the estimator and the summarizers share (mdnn.InputNorm, mdnn.RffBandwidth,
kme.KernelMeanEmbedding): a quantity made once on the device from the first chunk's training rows -- or given,
or loaded -- then frozen, kept in ``state_dict`` and refused under data parallel until it exists."""
import torch
from torch import nn

from . import _lib


class FrozenStatistic(nn.Module):
    """The given buffers, in their order, then ``count`` (int64 scalar: the number of rows or trajectories the
    value was made from, 0: not there yet).  The buffers follow the module to its device and keep their dtypes
    through ``.float()`` / ``.double()``.  ``ready`` is the host's copy of ``count > 0``: asking costs no
    read-back.  A subclass gives the two messages and may override ``_value_changed``."""
    NOT_READY = None           # require_ready's RuntimeError
    NOT_READY_PARALLEL = None  # refuse_data_parallel's ValueError

    def __init__(self, device, **buffers):
        super().__init__()
        for name, value in buffers.items():
            self.register_buffer(name, value.to(device))
        self.register_buffer('count', torch.zeros((), dtype=torch.int64, device=device))
        self.ready = False

    def _apply(self, fn, *args, **kwargs):
        # a change of device is followed, a change of dtype is not
        for name, buf in list(self._buffers.items()):
            self._buffers[name] = buf.to(fn(buf).device)
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + 'count' in state_dict:
            self.ready = int(state_dict[prefix + 'count']) > 0
        self._value_changed()

    def _value_changed(self):
        """The value has been made, given or loaded: what was derived from an earlier one is stale."""

    def made_from(self, n):
        """The value has just been written (on the stream, or from the host): ``count`` follows on the stream."""
        self.count.fill_(n)
        self.ready = True
        self._value_changed()

    def reset(self):
        """Back to "not there yet": the value that was made is not to be used."""
        self.count.zero_()
        self.ready = False

    def require_ready(self):
        if not self.ready:
            raise RuntimeError(self.NOT_READY)
        return self

    def refuse_data_parallel(self, dp):
        """Every rank of the group ``dp`` (None: no data parallel) would make the value from its own first chunk."""
        if dp is not None and not self.ready:
            raise ValueError(self.NOT_READY_PARALLEL)


def column_statistics(prec, xs, ld, n, width, mean, inv_std, workspace):
    """mean / inv_std (float64 ``[width]`` on the rows' device) <- the statistics of the first ``n`` rows of ``xs``
    (device rows of ``prec``'s dtype at pitch ``ld``): bsig_input_norm_stats, the flat rule of
    include/bsig_input_norm.h.  ``workspace(numel)`` gives a float64 device tensor of that many elements or more:
    the caller's own buffer policy.  Asynchronous; the caller has made the rows' device the current one."""
    need = int(_lib.load().bsig_input_norm_workspace_bytes(n, width))
    assert need > 0, 'input statistics need at least one row'
    ws = workspace(need // 8)
    prec.input_norm_stats(_lib.ptr(xs), ld, n, width, _lib.ptr(mean), _lib.ptr(inv_std), _lib.ptr(ws),
                          ws.numel() * 8, _lib.stream())
