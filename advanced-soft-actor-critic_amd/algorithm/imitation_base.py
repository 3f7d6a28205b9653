"""`ImitationBase` — behaviour cloning on whole demonstration episodes, the drop-in for the reference's
`algorithm/imitation_base.ImitationBase` (`imitation_base.py:12-73`): it pre-trains the representation and the policy of
an existing `SAC_Base` before, or between, SAC steps.

One `train(ep_obses_list, ep_actions, ep_rewards, ep_dones)`:
  1. the episode [1, T, *] is staged into static buffers of its bucket length Tp (`bucket_length`: the next multiple of 64):
     rows >= T get index -1, padding_mask True, zero observations and actions; row T - 1 keeps the reference's True mask
  2. zero the `rep` and `policy` gradient segments, representation forward over [1, Tp, *], policy forward
  3. `asac_bc_loss_grad` (csrc/imitation.hip): mean(-log_prob(a_c) - 0.1 * entropy) over the T valid rows and its gradients
     in one launch, T read from device memory; the stock policy's head transform rides in the same launch
  4. backward through policy and representation (the learner's fused modules, direct gradient accumulation, deferred
     partial sums), Adam on the two spans (two launches: the critics lie between them and are not swept), counters
Steps 2-4 have no host synchronisation: per bucket they are captured into one hipGraph after the first (eager) use and
replayed afterwards; `hip_config={'use_graph': False}` keeps them eager.  At most `hip_config['imitation_max_graphs']`
(default 8) bucket graphs are alive, the oldest is dropped first.  `hip_config['imitation_bucket']` (default 64) is the
bucket multiple (1: no padding); `hip_config['imitation_fused_head']` (default True) the stock policy's one-launch form.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from asac_amd import native

from .captured_step import CapturedStep
from .param_grads import learner_backward


ENTROPY_COEF = 0.1      # imitation_base.py:58
BUCKET = 64


def bucket_length(ep_len: int, multiple: int = BUCKET) -> int:
    """the padded length an episode of `ep_len` steps trains at: the next multiple of `multiple`, at least `multiple`"""
    if ep_len < 1:
        raise ValueError(f'an episode needs at least one step, got {ep_len}')
    multiple = max(int(multiple), 1)
    return (int(ep_len) + multiple - 1) // multiple * multiple


def bc_loss_terms(loc, scale, action, entropy_coef: float = ENTROPY_COEF):
    """The per-element loss and its gradients as `asac_bc_loss_grad` forms them (before the 1 / (T A) of the mean), in
    the tensors' own precision: -> (l, dl/dloc, dl/dscale)."""
    z = (action - loc) / scale
    half_log_2pi = 0.5 * float(np.log(2 * np.pi))
    log_s = torch.log(scale)
    loss = 0.5 * z * z + log_s + half_log_2pi - entropy_coef * (0.5 + half_log_2pi + log_s)
    return loss, -z / scale, (1 - entropy_coef - z * z) / scale


class _BcLossFn(torch.autograd.Function):
    """(loc, scale) of any Normal the policy returned -> the scalar loss; both gradients come out of the forward's launch"""

    @staticmethod
    def forward(ctx, loc, scale, action, action_offset, t_valid, entropy_coef):
        A = loc.shape[-1]
        l2, s2 = loc.detach().reshape(-1, A), scale.detach().reshape(-1, A)
        if l2.stride(-1) != 1 or s2.stride(-1) != 1 or l2.stride(0) != s2.stride(0):
            l2, s2 = l2.contiguous(), s2.contiguous()
        g = torch.empty((2, l2.shape[0], A), dtype=torch.float32, device=loc.device)
        loss = torch.empty(1, dtype=torch.float32, device=loc.device)
        native.bc_loss_grad(l2, s2, action.reshape(-1, action.shape[-1]), action_offset, t_valid, entropy_coef, loss,
                            g[0], g[1])
        ctx.save_for_backward(g)
        ctx.shape = loc.shape
        return loss.view(())

    @staticmethod
    def backward(ctx, g_loss):
        from .sac_aux import _is_unit
        (g,) = ctx.saved_tensors
        if not _is_unit(g_loss):
            g = g * g_loss
        return g[0].view(ctx.shape), g[1].view(ctx.shape), None, None, None, None


class _BcLossRawFn(torch.autograd.Function):
    """the stock policy's raw head outputs [rows, 2A] (mean | logstd) -> the scalar loss: the head transform and its
    chain rule run inside the loss launch, the gradient has the layout the fused MLP backward reads"""

    @staticmethod
    def forward(ctx, raw, action, action_offset, t_valid, entropy_coef):
        A = raw.shape[-1] // 2
        r = raw.detach()
        assert r.dim() == 2 and r.is_contiguous()
        g = torch.empty_like(r)
        loss = torch.empty(1, dtype=torch.float32, device=raw.device)
        native.bc_loss_grad(r[:, :A], r[:, A:], action.reshape(-1, action.shape[-1]), action_offset, t_valid, entropy_coef,
                            loss, g[:, :A], g[:, A:], raw_head=True)
        ctx.save_for_backward(g)
        return loss.view(())

    @staticmethod
    def backward(ctx, g_loss):
        from .sac_aux import _is_unit
        (g,) = ctx.saved_tensors
        return (g if _is_unit(g_loss) else g * g_loss), None, None, None, None


def bc_loss(loc, scale, action, action_offset, t_valid, entropy_coef: float = ENTROPY_COEF):
    """mean over the first `t_valid` rows of -Normal(loc, scale).log_prob(action[..., action_offset:]) - entropy_coef *
    entropy, differentiable with respect to loc and scale (`asac_bc_loss_grad`).  loc, scale: [..., A] device tensors,
    action [..., >= action_offset + A] with the same leading shape, t_valid: device int32[1]."""
    return _BcLossFn.apply(loc, scale, action, action_offset, t_valid, entropy_coef)


class SpanAdam:
    """Adam (torch defaults, as `FlatAdam`) with moments and a step count of its own over several segments of the learner's
    flat buffer that need not be adjacent: one launch per segment, nothing in between is touched.  The moment buffers hold
    the segments back to back (`_at[name]`: a segment's offset in them), so they are as long as the segments, not as the
    learner's flat buffer."""

    def __init__(self, group, names, lr, betas=(0.9, 0.999), eps=1e-8):
        dev = group.flat.device
        self.group, self.names = group, list(names)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.steps_done = torch.zeros(1, dtype=torch.int64, device=dev)
        self._at, total = {}, 0
        for n in self.names:
            s, e = group.span(n)
            self._at[n] = total
            total += e - s
        self.exp_avg = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.spans = [(group.span(n), self._at[n]) for n in self.names if group.span(n)[1] > group.span(n)[0]]

    def step(self) -> None:
        g = self.group
        for (s, e), at in self.spans:
            native.adam_step(g.flat[s:e], g.grad[s:e], self.exp_avg[at:at + e - s], self.exp_avg_sq[at:at + e - s], self.lr,
                             self.betas[0], self.betas[1], self.eps, self.steps_done)
        self.steps_done.add_(1)

    def zero_grad(self) -> None:
        for (s, e), _ in self.spans:
            self.group.grad[s:e].zero_()

    # -- torch.optim.Adam-compatible checkpoint format (parameter order: the segments in turn, as FlatAdam's) --------------
    def _param_list(self):
        return [p for n in self.names for p in self.group.params[n]]

    def _param_slots(self):
        """-> (parameter, its offset in the moment buffers), in checkpoint order"""
        for n in self.names:
            off = self._at[n]
            for p in self.group.params[n]:
                yield p, off
                off += p.numel()

    def state_dict(self) -> dict:
        step = self.steps_done.detach().to('cpu', torch.float32).reshape(())
        state, idx = {}, 0
        for idx, (p, off) in enumerate(self._param_slots()):
            if int(step.item()) > 0:
                k = p.numel()
                state[idx] = {'step': step.clone(), 'exp_avg': self.exp_avg[off:off + k].view(p.shape).clone(),
                              'exp_avg_sq': self.exp_avg_sq[off:off + k].view(p.shape).clone()}
        return {'state': state,
                'param_groups': [{'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': 0,
                                  'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False,
                                  'differentiable': False, 'fused': None, 'decoupled_weight_decay': False,
                                  'params': list(range(len(self._param_list())))}]}

    def load_state_dict(self, sd: dict) -> None:
        for idx, (p, off) in enumerate(self._param_slots()):
            st = sd['state'].get(idx)
            if st is not None:
                k = p.numel()
                self.exp_avg[off:off + k].copy_(st['exp_avg'].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(st['exp_avg_sq'].reshape(-1))
                self.steps_done.fill_(int(float(st['step'])))


class _Bucket:
    """the static inputs of one padded length (stable addresses for graph replay) and the graph captured over them"""

    def __init__(self, sac, Tp):
        dev = sac.device
        A_all = sac.d_action_summed_size + sac.c_action_size
        self.Tp = Tp
        self.index = torch.full((1, Tp), -1, dtype=torch.int32, device=dev)
        self.pad = torch.ones((1, Tp), dtype=torch.bool, device=dev)
        self.obs = [torch.zeros((1, Tp, *s), dtype=torch.float32, device=dev) for s in sac.obs_shapes]
        self.action = torch.zeros((1, Tp, A_all), dtype=torch.float32, device=dev)
        self.pre_action = torch.zeros((1, Tp, A_all), dtype=torch.float32, device=dev)
        self.hidden = torch.zeros((1, Tp, *sac.seq_hidden_state_shape), dtype=torch.float32, device=dev)
        self.t_valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.uses, self.last_T = 0, None      # (last_T: the valid length staged last, None before the first episode)
        self.graph, self.graph_failed = None, False      # (graph: a CapturedStep whose payload is the step's loss tensor)


def _as_device(x, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'expected a NumPy array or a tensor, got {type(x).__name__}')
    return t.to(device=device, dtype=dtype, non_blocking=True)


class ImitationBase:
    def __init__(self, sac_base):
        sac = self._sac = sac_base
        if not sac.c_action_size:
            raise ValueError('ImitationBase clones the continuous action head: with c_action_size == 0 its loss is a mean '
                             'over no elements (NaN on the reference, imitation_base.py:57-59) and nothing would train')
        if getattr(sac, '_dist', None) is not None:
            raise ValueError("ImitationBase is single-GPU: a data-parallel context (hip_config['dist']) is not supported "
                             'with it')
        cfg = dict(sac._kwargs.get('hip_config') or {})
        self._bucket_multiple = int(cfg.get('imitation_bucket', BUCKET))
        self._max_graphs = int(cfg.get('imitation_max_graphs', 8))
        if self._max_graphs < 1:
            raise ValueError("hip_config['imitation_max_graphs'] must be at least 1")
        self._use_graph = sac._use_graph
        self.opt = SpanAdam(sac._params, ['rep', 'policy'], sac.learning_rate)
        # the stock policy runs through a StockMLP of this object's own (same parameters and gradient views as the learner's
        # `_fpi`): nothing an imitation step does — cached workspaces that grow with the episode length — can reach the
        # instance whose buffers a captured SAC step holds by address.  Default: its head left raw (mean | logstd),
        # `asac_bc_loss_grad` applies the head itself; `imitation_fused_head=False`: its (loc | scale) output behind the
        # general loss function
        self._fpi_raw = self._fpi_ls = None
        if sac._fpi is not None:
            from .fused_mlp import StockMLP
            raw = bool(cfg.get('imitation_fused_head', True))
            desc = native.MlpDesc.from_buffer_copy(sac._fpi.desc)
            if raw:
                desc.head_transform = 0
            start, stop = sac._params.span('policy')
            own = StockMLP(desc, sac._params.flat, sac._params.grad, start, stop - start, 1, sac.device,
                           list(sac.model_policy.parameters()))
            self._fpi_raw, self._fpi_ls = (own, None) if raw else (None, own)
        self._buckets = OrderedDict()       # Tp -> _Bucket, oldest first
        self.captures = 0                   # hipGraphs captured so far (evicted ones included)
        self.capture_failures = 0           # buckets whose capture failed (they run eagerly)
        self._graph_failed = False
        self._graph_hp = None
        self._last_loss = None
        from .sac_aux import unit_gradient
        self._unit = unit_gradient(sac._params.flat)      # (made outside any capture: every graph shares it)
        native.bc_loss_grad_workspace(sac.device)

    # -- the step ------------------------------------------------------------------------------------------------------
    @property
    def last_loss(self):
        """the loss of the last `train` as a 0-d device tensor (reading it synchronises)"""
        return self._last_loss

    def _device_step(self, bk) -> torch.Tensor:
        """Everything one imitation step does on the device, on the bucket's static buffers: no host synchronisation"""
        from .fused_mlp import StockMLP
        from .nn_models.layers.seq_layers import step_mask_cache
        from .utils.enums import SEQ_ENCODER
        sac = self._sac
        self.opt.zero_grad()
        attn = sac.seq_encoder == SEQ_ENCODER.ATTN
        with step_mask_cache() if attn else contextlib.nullcontext():
            states, _ = sac.get_l_states(bk.index, bk.pad, bk.obs, bk.pre_action, bk.hidden, is_target=False)
            dsum = sac.d_action_summed_size
            if self._fpi_raw is not None:
                x = StockMLP._rows(states, sac.state_size)
                raw = self._fpi_raw(x).view(x.shape[0], 2 * sac.c_action_size)
                loss = _BcLossRawFn.apply(raw, bk.action, dsum, bk.t_valid, ENTROPY_COEF)
            elif self._fpi_ls is not None:
                A = sac.c_action_size
                x = StockMLP._rows(states, sac.state_size)
                ls = self._fpi_ls(x).view(x.shape[0], 2 * A)
                loss = bc_loss(ls[:, :A], ls[:, A:], bk.action, dsum, bk.t_valid, ENTROPY_COEF)
            else:
                _, c_policy, loc, scale, plain = sac._policy(states, bk.obs)
                if not plain:
                    raise TypeError('ImitationBase needs a policy whose continuous head is a torch.distributions.Normal, '
                                    f'got {type(c_policy).__name__}')
                loss = bc_loss(loc, scale, bk.action, dsum, bk.t_valid, ENTROPY_COEF)
            with learner_backward():
                loss.backward(self._unit)
        self.opt.step()
        return loss.detach()

    def _stage(self, bk, T, obses, actions) -> None:
        bk.index[0, :T].copy_(self._arange(T))
        bk.pad[0, :T - 1] = False
        if bk.last_T is not None and bk.last_T != T:
            bk.index[0, T:] = -1
            bk.pad[0, T - 1:] = True
        for dst, src in zip(bk.obs, obses):
            dst[0, :T].copy_(src[0], non_blocking=True)
            if bk.last_T is not None and bk.last_T > T:
                dst[0, T:bk.last_T].zero_()
        bk.action[0, :T].copy_(actions[0], non_blocking=True)
        bk.pre_action[0, 1:T].copy_(bk.action[0, :T - 1])      # gen_n_pre_actions(keep_last_action=False): zeros first
        if bk.last_T is not None and bk.last_T > T:
            bk.action[0, T:bk.last_T].zero_()
            bk.pre_action[0, T:bk.last_T].zero_()
        bk.t_valid.fill_(T)
        bk.last_T = T

    def _arange(self, T):
        ar = getattr(self, '_ar', None)
        if ar is None or ar.numel() < T:
            ar = self._ar = torch.arange(bucket_length(T, 1024), dtype=torch.int32, device=self._sac.device)
        return ar[:T]

    def _bucket_for(self, Tp):
        bk = self._buckets.get(Tp)
        if bk is None:
            while len(self._buckets) >= self._max_graphs:
                # the oldest bucket, its static buffers and its graph: a replay of it may still be running, and an
                # executable graph must not be destroyed under one — wait first (an eviction is a rare event)
                torch.cuda.synchronize(self._sac.device)
                self._buckets.popitem(last=False)
            bk = self._buckets[Tp] = _Bucket(self._sac, Tp)
        return bk

    def _capture(self, bk) -> None:
        sac = self._sac
        if not CapturedStep.api_ok():
            self._graph_failed = True       # (a property of the torch build: no bucket can be captured)
            sac._logger.warning('this torch build cannot repair captured memset nodes: imitation steps run eagerly')
            return
        try:
            bk.graph = CapturedStep.capture(lambda: self._device_step(bk), sac.device, logger=sac._logger)
            self.captures += 1
        except Exception as e:
            # a user model with a host synchronisation etc.: THIS bucket stays eager (as the learner's step does after a
            # failed capture), loudly; `capture_failures` counts them for callers that want to treat it as an error
            bk.graph_failed, bk.graph = True, None
            self.capture_failures += 1
            torch.cuda.synchronize()
            sac._logger.warning(f'hipGraph capture of the imitation step (episodes padded to {bk.Tp}) failed; these '
                                f'episodes run eagerly, several times slower: {e!r}')

    def _train_one(self, ep_obses_list, ep_actions) -> None:
        sac = self._sac
        dev = sac.device
        actions = _as_device(ep_actions, dev, torch.float32)
        if actions.dim() != 3 or actions.shape[0] != 1:
            raise ValueError(f'ep_actions must be [1, ep_len, action_size], got {tuple(actions.shape)}')
        T = actions.shape[1]
        obses = [_as_device(o, dev) for o in ep_obses_list]
        if len(obses) != len(sac.obs_shapes):
            raise ValueError(f'{len(sac.obs_shapes)} observations expected, got {len(obses)}')
        for name, o in zip(sac.obs_names, obses):
            # the reference hands the arrays to the representation as they are (imitation_base.py:41, no / 255 widening)
            if o.dtype != torch.float32:
                raise TypeError(f'observation {name!r} is {o.dtype}: ImitationBase takes float32 observations (widen 8-bit '
                                'images to [0, 1] floats first, as the learner does for replayed ones)')
        Tp = bucket_length(T, self._bucket_multiple)
        if Tp * sac.c_action_size > native.BC_MAX_ELEMENTS:
            raise ValueError(f'episode of {T} steps is too long for one imitation step')
        hp = (self.opt.lr, tuple(self.opt.betas), self.opt.eps)
        if hp != self._graph_hp:        # a captured step holds them as kernel arguments
            for b in self._buckets.values():
                b.graph = None
            self._graph_hp = hp
        bk = self._bucket_for(Tp)
        with torch.cuda.device(dev):
            self._stage(bk, T, obses, actions)
            graph_ok = self._use_graph and not self._graph_failed and not bk.graph_failed
            if graph_ok and bk.graph is not None:
                bk.graph.replay(direct=sac._direct_graph_launch)
                self._last_loss = bk.graph.payload
            else:
                self._last_loss = self._device_step(bk)
                if graph_ok and bk.graph is None:
                    self._capture(bk)       # replayed from the bucket's next episode on
        bk.uses += 1

    def _after_step(self) -> int:
        """imitation_base.py:64-73: summary, checkpoint, global step"""
        sac = self._sac
        if sac.get_global_step() % sac.write_summary_per_step == 0 and sac.summary_writer is not None:
            sac.write_constant_summaries([{'tag': 'offline/loss', 'simple_value': self._last_loss}])
        if sac.get_global_step() % sac.save_model_per_step == 0:
            sac.save_model()
        return sac.increase_global_step()

    def train(self, ep_obses_list, ep_actions, ep_rewards, ep_dones) -> int:
        """
        Args:
            ep_obses_list: list([1, ep_len, *obs_shapes_i], ...)   NumPy arrays or tensors (device tensors stay in HBM)
            ep_actions: [1, ep_len, action_size]
            ep_rewards: [1, ep_len]      (not read, as on the reference)
            ep_dones: [1, ep_len]        (not read, as on the reference)
        Returns the learner's global step after this one.
        """
        self._train_one(ep_obses_list, ep_actions)
        return self._after_step()

    def train_episodes(self, episodes) -> int:
        """`train` for every (ep_obses_list, ep_actions, ep_rewards, ep_dones) of `episodes`, back to back: with device
        tensors nothing between two episodes waits for the device (summaries and checkpoints still do, when due)"""
        step = self._sac.get_global_step()
        for ep in episodes:
            self._train_one(ep[0], ep[1])
            step = self._after_step()
        return step

    # -- torch.optim.Adam checkpoint format (as FlatAdam's: the reference can load it) ------------------------------------
    def state_dict(self) -> dict:
        return self.opt.state_dict()

    def load_state_dict(self, sd: dict) -> None:
        self.opt.load_state_dict(sd)
