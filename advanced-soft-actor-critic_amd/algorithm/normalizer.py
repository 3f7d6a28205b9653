"""Running observation statistics of `use_normalization` (reference sac_base.py:302-336, 766-781) and their two launches:
`asac_obs_whiten` (all observations of a call, one launch) and `asac_normalizer_update` (all observations of an episode,
one launch) — csrc/normalize.hip, behind `hip_config['fused_normalizer']`.

All means and variances are views of ONE flat float32 buffer; `running_means[i]`, `running_variances[i]` and
`normalizer_step` keep the names, shapes, dtypes and initial values (zeros, ones, int32 0) of the eager path, so a
checkpoint of either path loads into the other.  Job tables are host structures built once per set of buffers and kept with
the tensors they point into: a replayed step builds nothing, a capture contains the whiten launch and nothing else.
Whatever the launches do not take — CPU tensors, other dtypes, more than `native.NORM_MAX_OBS` observations, a non-unit
innermost stride — runs the module expression / the eager update, silently."""
import numpy as np
import torch

from asac_amd import native


def fused_normalizer_applies(*, enabled, use_normalization, plain_learner, data_parallel, float32_on_device) -> bool:
    """Does a learner of this configuration whiten its observations in front of the representation with one
    `asac_obs_whiten` launch a step and keep its statistics with `asac_normalizer_update`
    (`hip_config['fused_normalizer']`, default off)?  Only a plain `SAC_Base` (`plain_learner`: not an `OptionBase`) with
    `use_normalization`, without a data-parallel context, on float32 device parameters.  Everything else keeps the
    `NormalizedRep` subclass and the eager update."""
    return bool(enabled and use_normalization and plain_learner and not data_parallel and float32_on_device)


def whiten_expression(obs_list, means, variances, step):
    """the module expression (reference sac_base.py:318-322)"""
    return [torch.clamp((o - m) / torch.sqrt(v / (step + 1)), -5, 5) for o, m, v in zip(obs_list, means, variances)]


@torch.no_grad()
def update_expression(obs_list, means, variances, step) -> None:
    """the eager update (reference sac_base.py:766-781)"""
    step.add_(obs_list[0].shape[0])
    for obs, mean, var in zip(obs_list, means, variances):
        to_old = obs - mean
        new_mean = mean + torch.sum(to_old / step, dim=0)
        new_var = var + torch.sum((obs - new_mean) * to_old, dim=0)
        mean.copy_(new_mean)
        var.copy_(new_var)


def _layout(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)


class Normalizer:
    def __init__(self, obs_shapes, device):
        self.obs_shapes = [tuple(s) for s in obs_shapes]
        sizes = [int(np.prod(s)) if len(s) else 1 for s in self.obs_shapes]
        # (every view starts on a 16-byte boundary: the whiten launch reads the statistics four at a time)
        starts, total = [], 0
        for n in sizes * 2:
            starts.append(total)
            total += (n + 3) // 4 * 4
        k = len(sizes)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.running_means = [self.flat[o:o + n].view(s) for o, n, s in zip(starts[:k], sizes, self.obs_shapes)]
        self.running_variances = [self.flat[o:o + n].view(s) for o, n, s in zip(starts[k:], sizes, self.obs_shapes)]
        for v in self.running_variances:
            v.fill_(1.)
        self.normalizer_step = torch.tensor(0, dtype=torch.int32, device=device, requires_grad=False)
        # the update's arrival counter (asac_ordered_finish.h): zero before first use, left zero by every launch
        self._counter = torch.zeros(1, dtype=torch.int32, device=device) if self.flat.is_cuda else None
        self._tables = {}       # layouts of (sources, destinations) -> (job table, destinations, sources)
        self._static_out = {}   # shapes of a static set -> its whitened buffers
        self.whitened = None    # the destination buffers of the last `whiten` call that launched

    # ------------------------------------------------------------------------------------------
    def _native_obs(self, obs_list) -> bool:
        return (self.flat.is_cuda and 1 <= len(obs_list) <= native.NORM_MAX_OBS and len(obs_list) == len(self.obs_shapes)
                and all(isinstance(o, torch.Tensor) and o.is_cuda and o.numel() > 0
                        and (o.dim() == 0 or o.stride(-1) == 1 or o.shape[-1] == 1)
                        and tuple(o.shape[o.dim() - len(s):]) == s for o, s in zip(obs_list, self.obs_shapes)))

    @torch.no_grad()
    def whiten(self, obs_list, out=None, static=False):
        """-> the whitened observations.  `out`: a list of buffers of the observations' shapes (an observation itself: in
        place), default fresh ones.  `static`: the observations are static buffers (the learner's batch): their job table
        and, without `out`, their whitened buffers are made on the first call and kept for good — later calls, replayed or
        captured, build nothing"""
        obs_list = list(obs_list)
        if not (self._native_obs(obs_list) and all(o.dtype == torch.float32 for o in obs_list)):
            return self._whiten_eager(obs_list, out)
        key = entry = None
        if static:
            key = tuple(_layout(o) for o in obs_list) + (None if out is None else tuple(_layout(o) for o in out),)
            entry = self._tables.get(key)
        if entry is None:
            if static and torch.cuda.is_current_stream_capturing():
                raise native.AsacNativeError('Normalizer.whiten: static buffers first seen inside a capture')
            if out is not None:
                dst = list(out)
            elif static:
                # static sets of one shape (the two sets of `hip_config['lookahead']`) share their whitened buffers: a step
                # whitens the batch it trains on and reads the result before the next step's launch writes it
                dst = self._static_out.setdefault(tuple(tuple(o.shape) for o in obs_list), [
                    torch.empty(o.shape, dtype=torch.float32, device=o.device) for o in obs_list])
            else:
                dst = [torch.empty(o.shape, dtype=torch.float32, device=o.device) for o in obs_list]
            jobs = native.whiten_jobs(list(zip(obs_list, dst, self.running_means, self.running_variances)))
            if jobs is None:
                return self._whiten_eager(obs_list, out)
            entry = (jobs, dst, obs_list)
            if static:
                self._tables[key] = entry
        jobs, dst, _ = entry
        native.obs_whiten(jobs, self.normalizer_step)
        self.whitened = dst
        return dst

    def _whiten_eager(self, obs_list, out):
        res = whiten_expression(obs_list, self.running_means, self.running_variances, self.normalizer_step)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return list(out)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, obs_list) -> None:
        """the statistics over an episode's rows `obs_list[i]` [T, *obs_shapes[i]], and `normalizer_step += T`"""
        obs_list = list(obs_list)
        dtypes = {torch.float32: native.NORM_F32, torch.uint8: native.NORM_U8}
        if not (self._native_obs(obs_list) and all(o.dtype in dtypes and o.dim() == 1 + len(s) and o.shape[0] == obs_list[0].shape[0]
                                                   for o, s in zip(obs_list, self.obs_shapes))):
            return update_expression(obs_list, self.running_means, self.running_variances, self.normalizer_step)
        jobs = (native.NormalizerJob * len(obs_list))()
        for slot, o, mean, var in zip(jobs, obs_list, self.running_means, self.running_variances):
            pitch = native._row_pitch(o, mean.dim(), mean.numel())
            if pitch is None:
                return update_expression(obs_list, self.running_means, self.running_variances, self.normalizer_step)
            slot.x, slot.mean, slot.variance = o.data_ptr(), mean.data_ptr(), var.data_ptr()
            slot.D, slot.x_row_pitch, slot.dtype = mean.numel(), pitch, dtypes[o.dtype]
        native.normalizer_update(jobs, obs_list[0].shape[0], self.normalizer_step, self._counter)
