"""`SAC_Base` — the drop-in learner for reference `algorithm/sac_base.SAC_Base`
(`/root/reference/algorithm/sac_base.py:19-2614`) with its training step re-built for MI355X.

Same constructor keywords (every `sac_config` key of the reference's `default_config.yaml`), same
model-plugin protocol (`nn.ModelRep / ModelQ / ModelPolicy ...`), same public methods
(`train`, `put_episode`, `choose_action`, `choose_attn_action`, `save_model`, ...).

How one `train()` runs here (reference call stack: SURVEY.md §3.1):
  1. PER sample + window gather + padding      2 HIP launches, data never leaves HBM
  2. Polyak soft update                         1 launch over the flat target / online buffers
  3. representation / Q / policy forward+backward on PyTorch-ROCm (rocBLAS / hipBLASLt -> MFMA)
  4. target value: rsample + tanh-squash log-prob, stored-action probabilities, ensemble subset
     min, V = minQ - alpha*logpi, V-trace scan      3 fused launches (`asac_squash_*`, `asac_vtrace_*`)
  5. clipped double-Q loss + its gradient       1 launch;  Adam per optimizer: 1 launch per segment
  6. TD error -> priority update, mu-prob / hidden-state write-back   fused launches, no D2H
The device work of a whole step has no host synchronisation, so after a few eager steps it is
captured into one hipGraph (torch.cuda.CUDAGraph) and replayed; `hip_config={'use_graph': False}`
keeps it eager.  Every random draw comes from `self.noise` (device Philox by default; tests inject
recorded draws to compare against the reference bit-for-bit on index selection).

`use_replay_buffer=False` trains from fresh episodes instead (reference BatchBuffer, batch_buffer.py): every
episode's windows go, shuffled and padded, into an HBM window pool in ONE launch (`asac_batch_put`), and step 1 above
becomes ONE launch that copies the oldest queued batch into the same static batch (`asac_batch_pop_gather`).  That mode
has no PER draws, no IS weights and no step 6 (the reference's `train` skips them too); the step is still one hipGraph.
"""
import contextlib
import logging
import random
from collections import defaultdict, namedtuple
from pathlib import Path

import numpy as np
import torch
from torch import distributions, nn
from torch.nn import functional

from asac_amd import native

from . import fused_gru, fused_linear
from .fused import DeviceNoise, FlatAdam, FlatParamGroup, squash_sample, squash_sample_ls, time_slice
from .fused_mlp import StockMLP, describe_policy, describe_q
from .nn_models import *  # noqa: F401,F403
from .nn_models.layers.seq_layers import step_mask_cache
from .nn_models.representation import ModelSimpleRep
from .normalizer import Normalizer, fused_normalizer_applies
from .param_grads import direct_param_grads, learner_backward
from .batch_buffer import BatchBuffer
from .captured_step import CapturedStep
from .replay_buffer import PrioritizedReplayBuffer
from .sac_aux import AuxHeadsMixin
from .utils import *  # noqa: F401,F403
from .utils.enums import CURIOSITY, SEQ_ENCODER, SIAMESE
from .utils.elapse_timer import UnifiedElapsedTimer, unified_elapsed_timer
from .utils.operators import (gen_n_pre_actions, squash_correction_log_prob,
                              squash_correction_prob, sum_entropy, sum_log_prob)

try:  # tensorboard is optional (absent on the GPU box image)
    from torch.utils.tensorboard import SummaryWriter
except Exception:  # pragma: no cover
    SummaryWriter = None


def _masked_mse_backward(pred, target, padding_mask, loss_out, fused=True):
    """loss = mean over ALL elements of (pred - target)^2 with padded rows zeroed (`mse_loss(reduction='none') *
    ~mask` then `mean`, reference sac_base.py:1962-1964) -> `loss_out`, and `loss.backward()` through `pred`:
    the loss is the root, so its gradient 2 d / N is handed to autograd directly (six launches in all)."""
    with torch.no_grad():
        if (fused and pred.is_cuda and pred.dim() == 3 and pred.dtype == torch.float32 and pred.is_contiguous()
                and target.stride(-1) == 1 and pred.numel() <= native.MASKED_MSE_MAX and padding_mask.dtype == torch.bool
                and (padding_mask.stride(1) == 1 or padding_mask.shape[1] == 1)):
            d = torch.empty_like(pred)
            native.masked_mse(pred.detach(), target, padding_mask, d, loss_out)       # one launch
        else:
            d = (pred - target).mul_((~padding_mask).unsqueeze(-1))
            flat = d.reshape(-1)
            torch.div(torch.dot(flat, flat), flat.numel(), out=loss_out)
            d.mul_(2. / flat.numel())
    with direct_param_grads():      # detached inputs: the backward reaches the model's own parameters only
        pred.backward(d)


def _real(x):
    """a concatenation that left the representation un-consumed (a plugin whose returned state IS a `torch.cat`) is
    formed here: nothing outside the representation ever sees an `adjacent_cat.DeferredCat`"""
    from .adjacent_cat import DeferredCat
    return x.materialize() if isinstance(x, DeferredCat) else x


# a captured k-step run (`train_steps`): the step graph it was captured beside, its CapturedStep (None: the capture failed)
_GraphRun = namedtuple('_GraphRun', 'beside run')
_Return = namedtuple('_Return', 'args keep')     # `SAC_Base._c_return`


def fused_discrete_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, discrete_dqn_like, offline_loss,
                           siamese, use_prediction, data_parallel, float32_on_device, ensemble_q_num, n_step,
                           batch_size) -> bool:
    """Does a step of this configuration run the pure-discrete, policy-based learner's arithmetic on the
    `asac_discrete_*` launches (`hip_config['fused_discrete']`)?  Only a plain `SAC_Base` step (`plain_learner`: not an
    `OptionBase`) with discrete branches alone and a policy (no DQN-like target), without an offline loss, a siamese or a
    prediction head or a data-parallel context, on float32 device tensors, within the entry points' size limits.
    Everything else runs the eager code."""
    return bool(enabled and plain_learner and len(d_action_sizes) > 0 and c_action_size == 0 and not discrete_dqn_like
                and not offline_loss and not siamese and not use_prediction and not data_parallel and float32_on_device
                and native.discrete_sizes_ok(d_action_sizes, ensemble_q_num, n_step, batch_size))


def fused_hybrid_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, discrete_dqn_like, offline_loss, siamese,
                         use_prediction, data_parallel, float32_on_device, clip_epsilon, plain_gaussian, ensemble_q_num,
                         n_step, batch_size) -> bool:
    """Does a step of this configuration run the policy-based learner's arithmetic of a HYBRID action space on the
    `asac_hybrid_*` launches (`hip_config['fused_hybrid']`, default off)?  Only a plain `SAC_Base` step (`plain_learner`:
    not an `OptionBase`) with discrete branches and continuous actions and a policy (no DQN-like target), without an offline
    loss, a siamese or a prediction head or a data-parallel context, on float32 device tensors, with the clipped Q loss
    (`clip_epsilon > 0`: the reference's doubling at 0 stays eager) and a continuous head that (loc, scale) fully describe
    (`plain_gaussian`), within the entry points' size limits.  Everything else runs the eager code."""
    return bool(enabled and plain_learner and len(d_action_sizes) > 0 and c_action_size > 0 and not discrete_dqn_like
                and not offline_loss and not siamese and not use_prediction and not data_parallel and float32_on_device
                and clip_epsilon > 0 and plain_gaussian
                and native.hybrid_sizes_ok(d_action_sizes, c_action_size, ensemble_q_num, n_step, batch_size))


def fused_dqn_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, discrete_dqn_like, offline_loss, siamese,
                      use_prediction, curiosity, data_parallel, float32_on_device, ensemble_q_num, n_step, batch_size) -> bool:
    """Does a step of this configuration run the pure-discrete, DQN-like learner's arithmetic on the `asac_dqn_*`
    launches (`hip_config['fused_dqn']`)?  Only a plain `SAC_Base` step (`plain_learner`: not an `OptionBase`) with
    discrete branches alone and `discrete_dqn_like`, without an offline loss, a siamese or a prediction head, curiosity or
    a data-parallel context, on float32 device tensors, within the entry points' size limits.  Everything else runs the
    eager code."""
    return bool(enabled and plain_learner and len(d_action_sizes) > 0 and c_action_size == 0 and discrete_dqn_like
                and not offline_loss and not siamese and not use_prediction and not curiosity and not data_parallel
                and float32_on_device and native.discrete_sizes_ok(d_action_sizes, ensemble_q_num, n_step, batch_size))


def fused_offline_applies(*, enabled, plain_learner, offline_loss, c_action_size, d_action_sizes, stock_networks,
                          data_parallel, float32_on_device) -> bool:
    """Does a continuous learner with the offline loss (`offline_enabled and offline_loss`: reference sac_base.py:1899-1900)
    keep the native continuous path, the loss' term riding in the policy-step launches
    (`hip_config['fused_offline']`)?  Only a plain `SAC_Base` (`plain_learner`: not an `OptionBase`) with continuous
    actions alone, stock Q and policy networks (`stock_networks`), without a data-parallel context, on float32 device
    parameters.  Everything else runs the eager code."""
    return bool(enabled and plain_learner and offline_loss and c_action_size > 0 and len(d_action_sizes) == 0
                and stock_networks and not data_parallel and float32_on_device)


def fused_rnd_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, data_parallel, float32_on_device, stack_ok,
                      state_size, n_sample=1, rows=1) -> bool:
    """Does random network distillation of this configuration run on the `asac_rnd_*` launches (`hip_config['fused_rnd']`)?
    Only a plain `SAC_Base` (`plain_learner`: not an `OptionBase`) with continuous actions alone, without a data-parallel
    context, on float32 device tensors, whose `model_rnd.c_dense` and `model_target_rnd.c_dense` are both the stock stack
    on 16-byte-aligned contiguous parameters (`stack_ok`), within the entry points' limits (`n_sample` candidates an
    entry when acting, `rows` = batch * window rows when training).  Everything else runs the eager code."""
    return bool(enabled and plain_learner and len(d_action_sizes) == 0 and c_action_size > 0 and not data_parallel
                and float32_on_device and stack_ok and native.rnd_sizes_ok(state_size, c_action_size, n_sample, rows))


def fused_rnd_discrete_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, discrete_dqn_like, data_parallel,
                               float32_on_device, stack_ok, state_size, n_sample=1, rows=1) -> bool:
    """Does random network distillation of this configuration run on the `asac_drnd_*` launches
    (`hip_config['fused_rnd_discrete']`)?  Only a plain `SAC_Base` (`plain_learner`: not an `OptionBase`) with discrete
    branches alone and a policy (`discrete_dqn_like=False`), without a data-parallel context, on float32 device tensors,
    whose `model_rnd.d_dense_list` and `model_target_rnd.d_dense_list` are all the stock stack on 16-byte-aligned contiguous
    parameters (`stack_ok`), within the entry points' limits (`n_sample` candidates an entry when acting, `rows` = batch *
    window rows when training).  Everything else — hybrid spaces, the DQN-like `s_dense` form — runs the eager code."""
    return bool(enabled and plain_learner and len(d_action_sizes) > 0 and c_action_size == 0 and not discrete_dqn_like
                and not data_parallel and float32_on_device and stack_ok
                and native.drnd_sizes_ok(state_size, d_action_sizes, n_sample, rows))


def fused_act_applies(*, enabled, plain_learner, d_action_sizes, c_action_size, discrete_dqn_like, rnd_in_effect,
                      offline_action, float32_on_device, state_dim) -> bool:
    """Does `_choose_action` of this configuration and this call turn the policy's head outputs into (action, prob) with
    the one `asac_act_policy` launch (`hip_config['fused_act']`)?  Only a plain `SAC_Base` (`plain_learner`: not an
    `OptionBase`) that acts on its policy (no DQN-like greedy acting), in a call where RND plays no part (`rnd_in_effect`:
    `use_rnd and (train_mode or force_rnd_if_available)`) and no `offline_action` is given, on float32 device parameters
    and a 2-D state, within the entry point's limits (`native.act_sizes_ok`).  Everything else runs the eager code.
    `_choose_action` asks this AFTER its four earlier one-launch branches: a stock continuous-only policy without
    `action_noise` satisfies this predicate too and is still served by the branch in front of it."""
    return bool(enabled and plain_learner and not discrete_dqn_like and not rnd_in_effect and not offline_action
                and float32_on_device and state_dim == 2 and native.act_sizes_ok(d_action_sizes, c_action_size))


def fused_siamese_applies(*, enabled, siamese, float32_on_device, N, n, widths, target_requires_grad) -> bool:
    """Do the siamese losses of this step run on the `asac_siamese_*` launches (`hip_config['fused_siamese']`, default off)?
    Only float32 device tensors whose target side carries no gradient, within the entry points' limits: ATC — every
    encoder width E in 1 .. 128, block length n in 1 .. 64 dividing the N = batch * n rows, N <= 16 384; BYOL — every
    prediction width P in 1 .. 256, N <= 2^20 (`widths`: the E of each encoder, or the P of each prediction).  Everything
    else runs the eager code."""
    if not (enabled and siamese is not None and float32_on_device and not target_requires_grad and len(widths) > 0):
        return False
    if siamese == SIAMESE.ATC:
        return bool(all(1 <= w <= native.SIAMESE_MAX_WIDTH for w in widths) and 1 <= n <= native.SIAMESE_MAX_BLOCK
                    and 1 <= N <= native.SIAMESE_MAX_ROWS and N % n == 0)
    if siamese == SIAMESE.BYOL:
        return bool(all(1 <= w <= native.SIAMESE_BYOL_MAX_WIDTH for w in widths) and 1 <= N <= native.SIAMESE_BYOL_MAX_ROWS)
    return False


class _Window:
    """views of the step's static batch tensors and what the phases of `_device_step_body` hand to each other"""


class _AfterPolicy:
    """what the stock networks' pass of the UPDATED policy over the window leaves for the temperature step, the TD
    error and the write-backs (all None: the generic path computes each where it is needed)"""
    ls_win = alpha_logp = probs_win = td_sample = None      # (loc | scale) [B, L, 2A]; log pi of the temperature sample;
    #                                                           pi(stored actions) [B, L, A]; the TD target's (action, log pi)
    sc_write = sc_alpha = None                               # sidecar jobs still waiting for a host launch
    td_riders = td_alpha = None                              # for the TD error's return launch (`_launch_return`): the
    #                                                           sidecar jobs it hosts, the temperature step it anticipates
    side_cq = td_q_table = ls_td = td_pi = None              # online Q(s_b, a_b); target Q on the TD sample; the TD
    #                                                           target's own policy pass (over target states) and its pi
    mu_written = False                                       # the mu-probability write-back is issued / riding


class SAC_Base(AuxHeadsMixin):
    _closed = False
    _plain_learner = True        # (OptionBase: False — the one-launch paths of the plain learner's arithmetic stay off)

    def __init__(self,
                 obs_names: list[str],
                 obs_shapes: list[tuple[int]],
                 d_action_sizes: list[int],
                 c_action_size: int,
                 model_abs_dir: Path | None,
                 nn,

                 device: str | None = None,
                 ma_name: str | None = None,
                 summary_path: str | None = 'log',
                 train_mode: bool = True,
                 last_ckpt: str | None = None,

                 nn_config: dict | None = None,

                 seed: float | None = None,
                 write_summary_per_step: float = 1e3,
                 save_model_per_step: float = 1e5,

                 use_replay_buffer: bool = True,
                 use_priority: bool = True,

                 ensemble_q_num: int = 2,
                 ensemble_q_sample: int = 2,

                 burn_in_step: int = 0,
                 n_step: int = 1,
                 seq_encoder: SEQ_ENCODER | None = None,

                 batch_size: int = 256,
                 tau: float = 0.005,
                 update_target_per_step: int = 1,
                 init_log_alpha: float = -2.3,
                 use_auto_alpha: bool = True,
                 target_d_alpha: float = 0.98,
                 target_c_alpha: float = 1.,
                 d_policy_entropy_penalty: float = 0.5,

                 learning_rate: float = 3e-4,

                 gamma: float = 0.99,
                 v_lambda: float = 1.,
                 v_rho: float = 1.,
                 v_c: float = 1.,
                 clip_epsilon: float = 0.2,

                 discrete_dqn_like: bool = False,
                 discrete_dqn_epsilon: float = 0.2,
                 use_n_step_is: bool = True,

                 siamese: SIAMESE | None = None,
                 siamese_use_q: bool = False,
                 siamese_use_adaptive: bool = False,

                 use_prediction: bool = False,
                 transition_kl: float = 0.8,
                 use_extra_data: bool = True,

                 curiosity: CURIOSITY | None = None,
                 curiosity_strength: float = 1.,
                 use_rnd: bool = False,
                 rnd_n_sample: int = 10,

                 use_normalization: bool = False,

                 offline_enabled: bool = False,
                 offline_loss: bool = False,

                 action_noise: list[float] | None = None,

                 replay_config: dict | None = None,
                 hip_config: dict | None = None):
        """Arguments as in the reference (`sac_base.py:22-164`).  `hip_config` is the one new,
        optional section: {'use_graph': bool (default True), 'graph_warmup': int (default 3),
        'fused_mlp': bool (default True: stock ModelQ / ModelPolicy run as fused MFMA kernels),
        'twin_rep': bool (default True: the online and the target representation's fused GRU passes over the
        sampled window share one launch, see `fused_gru.TwinPass`)}."""
        self._kwargs = {k: v for k, v in locals().items() if k != 'self'}

        self.obs_names = obs_names
        self.obs_shapes = obs_shapes
        self.d_action_sizes = d_action_sizes
        self.d_action_summed_size = sum(d_action_sizes)
        self.d_action_branch_size = len(d_action_sizes)
        self.c_action_size = c_action_size
        self.model_abs_dir = model_abs_dir
        self.ma_name = ma_name
        self.train_mode = train_mode

        self.use_replay_buffer = use_replay_buffer
        self.use_priority = use_priority
        self.ensemble_q_num = ensemble_q_num
        self.ensemble_q_sample = ensemble_q_sample
        self.burn_in_step = burn_in_step
        self.n_step = n_step
        self.seq_encoder = seq_encoder
        self.write_summary_per_step = int(write_summary_per_step)
        self.save_model_per_step = int(save_model_per_step)
        self.batch_size = batch_size
        self.tau = tau
        self.update_target_per_step = update_target_per_step
        self.use_auto_alpha = use_auto_alpha
        self.target_d_alpha = target_d_alpha
        self.target_c_alpha = target_c_alpha
        self.d_policy_entropy_penalty = d_policy_entropy_penalty
        self.learning_rate = learning_rate
        self.gamma = gamma
        self.v_lambda = v_lambda
        self.v_rho = v_rho
        self.v_c = v_c
        self.clip_epsilon = clip_epsilon
        self.discrete_dqn_like = discrete_dqn_like
        self.discrete_dqn_epsilon = discrete_dqn_epsilon
        self.use_n_step_is = use_n_step_is
        self.siamese = siamese
        self.siamese_use_q = siamese_use_q
        self.siamese_use_adaptive = siamese_use_adaptive
        self.use_prediction = use_prediction
        self.transition_kl = transition_kl
        self.use_extra_data = use_extra_data
        self.curiosity = curiosity
        self.curiosity_strength = curiosity_strength
        self.use_rnd = use_rnd
        self.rnd_n_sample = rnd_n_sample
        self.use_normalization = use_normalization
        self.offline_enabled = offline_enabled
        self.offline_loss = offline_loss
        self.action_noise = action_noise

        hip_config = dict(hip_config or {})
        self._use_graph = bool(hip_config.get('use_graph', True))
        self._graph_warmup = int(hip_config.get('graph_warmup', 3))
        self._direct_graph_launch = bool(hip_config.get('direct_graph_launch', True))   # (False: every replay through torch)
        self._dist = hip_config.get('dist')     # parallel.DataParallelContext or None
        self._use_fused_mlp = bool(hip_config.get('fused_mlp', True))
        self._graph_collectives = bool(hip_config.get('graph_collectives', True))
        self._twin_rep = bool(hip_config.get('twin_rep', True))
        self._fuse_linear_tanh = bool(hip_config.get('fused_linear_tanh', True))
        self._use_sidecars = bool(hip_config.get('sidecars', True))
        # batches of 257 .. 1 024: the IS weights in an extra workgroup of the gather's launch instead of behind an exchange
        # between the sampler's workgroups (asac_step_prologue_sample_partial + asac_window_gather_pad_w)
        self._defer_is_weights = bool(hip_config.get('defer_is_weights', True))
        self._fused_policy_step = bool(hip_config.get('fused_policy_step', True))
        self._fused_forward_chain = bool(hip_config.get('fused_forward_chain', True))
        self._fused_td_chain = bool(hip_config.get('fused_td_chain', True))
        self._fused_td_update = bool(hip_config.get('fused_td_update', True))
        self._fused_q_return = bool(hip_config.get('fused_q_return', True))
        # the policy step LOADS the policy's forward a rider of the Q-loss backward launch saved (`_stock_q_backward`)
        self._policy_forward_rider = bool(hip_config.get('policy_forward_rider', True))
        # the Q-loss backward LOADS the online critics' forward a rider of the step's first network launch saved
        # (`_train_rep_q_stock`, `_critic_rider_plan`)
        self._critic_forward_rider = bool(hip_config.get('critic_forward_rider', True))
        self._fused_q_state_grads = bool(hip_config.get('fused_q_state_grads', True))
        self._gru_backward_at = bool(hip_config.get('gru_backward_at', True))
        self._adjacent_cat = bool(hip_config.get('adjacent_cat', True))
        self._fold_rep_q_adam = bool(hip_config.get('fold_rep_q_adam', True))
        self._rep_grad_one_position = bool(hip_config.get('rep_grad_one_position', True))
        self._deferred_cat = bool(hip_config.get('deferred_cat', True))
        self._rep_from_burn_in = bool(hip_config.get('rep_from_burn_in', True))
        self._fused_curiosity = bool(hip_config.get('fused_curiosity', True))
        self._fused_discrete = bool(hip_config.get('fused_discrete', True))     # asac_discrete_* (pure-discrete learner)
        self._fused_dqn = bool(hip_config.get('fused_dqn', True))               # asac_dqn_* (DQN-like discrete learner)
        self._fused_rnd = bool(hip_config.get('fused_rnd', True))               # asac_rnd_* (continuous RND, stock stacks)
        self._fused_offline = bool(hip_config.get('fused_offline', True))       # the offline loss inside the policy-step launches
        self._rnd_stacks = None          # (RndDesc, predictor, target, tensors) | False once described (`_rnd_fused`)
        self._rnd_buffers = {}           # (B, n) -> the distillation launch's dense outputs
        # asac_drnd_* (pure-discrete RND with a policy, stock stacks): NOTES.md, "discrete RND"
        self._fused_rnd_discrete = bool(hip_config.get('fused_rnd_discrete', True))
        self._drnd_stacks = None         # (residual, predictor table, target table, gradient table, tensors) | False (`_drnd_fused`)
        self._drnd_buffers = {}          # (B, n) -> the distillation launch's records and both launches' exchange words
        self._fused_act = bool(hip_config.get('fused_act', True))               # asac_act_policy (policy-based acting)
        # asac_siamese_* (ATC / BYOL loss and gradients as one launch an encoder); off by default: NOTES.md, "siamese losses"
        self._fused_siamese = bool(hip_config.get('fused_siamese', False))
        # asac_hybrid_* (hybrid action spaces).  Off by default: the default learner's hybrid step is held to the
        # `step/hybrid/*` entries of tests/parity_tolerances.json, 4x the errors observed on the eager composition, and
        # another summation order cannot promise to stay inside them
        self._fused_hybrid = bool(hip_config.get('fused_hybrid', False))
        # asac_obs_whiten / asac_normalizer_update (`use_normalization`: the learner whitens once a step in front of the
        # plugin's own representation class, algorithm/normalizer.py).  Off by default: the default learner's normalized step
        # is held to the recorded tolerances of the `aux_norm` golden case, and another summation order in the statistics
        # cannot promise to stay inside them
        self._fused_normalizer = bool(hip_config.get('fused_normalizer', False))
        # asac_head_bank_* (the discrete branch stacks of the stock critics and policy as one launch per pass,
        # algorithm/fused_heads.py).  Off by default: the discrete, DQN-like, hybrid and option steps are held to tolerances
        # recorded on the module path, and another summation order cannot promise to stay inside them
        self._fused_discrete_nets = bool(hip_config.get('fused_discrete_nets', False))
        self.normalizer = None
        self._siamese_ws = {}            # (N, E) / ('byol', encoder index) -> the launch's zeroed exchange words
        self._fused_rpm_loss = bool(hip_config.get('fused_rpm_loss', True))
        # one backward walk per prediction model (gates and model gradients from it): sac_aux._train_rpm
        self._rpm_single_backward = bool(hip_config.get('rpm_single_backward', True))
        self._fused_gating = bool(hip_config.get('fused_gating', True))          # asac_cosine_gate_add
        # the convolution stack's share of the three per-loss walks of `_train_rpm` as one launch (asac_conv2_backward_multi)
        self._rpm_conv_one_launch = bool(hip_config.get('rpm_conv_one_launch', True))
        # one sampled batch in flight, the reference's schedule (replay_buffer.py:275, 339-396): see `_step_sample`
        self._lookahead = int(hip_config.get('lookahead', 0))
        assert self._lookahead in (0, 1), 'hip_config lookahead: 0 (synchronous sampling) or 1 (one batch in flight)'
        # (graph branches — the next batch's draw, the target representation's pass — on a second stream were measured
        # slower than the launches in line and are gone: a fork / join inside a replayed hipGraph costs more than the small
        # launches it hides, NOTES.md section 1 rounds 4 / 5)
        self._la_gather_sidecar = bool(hip_config.get('lookahead_gather_sidecar', True)) and self._use_sidecars
        # the synchronous schedule's own gather as a rider of the step's first network launch, which reads its rows from
        # the replay ring (`_train_rep_q_stock`); False: the stand-alone gather launch in front of it
        self._head_gather_sidecar = bool(hip_config.get('head_gather_sidecar', True)) and self._use_sidecars
        self._head_gather = None      # the pending gather of the step's batch (`rb.head_gather`), until a launch takes it
        self._head_gather_w = False   # ... and the batch's IS weights are pending with it
        self._head_plan_cache = None  # (`rb._gather_keys` it was decided for, `rb.head_gather` or None): `_head_gather_plan`
        self._la_gather = None
        self._fuse_prediction_dense = bool(hip_config.get('fuse_prediction_dense', True))
        self._fused_q_loss_with_aux = bool(hip_config.get('fused_q_loss_with_aux', True))
        self._head_sums_members = bool(hip_config.get('head_sums_members', True))
        self._rep_epilogue, self._rep_epilogue_hp = False, None      # (False: not looked at yet; None: not applicable)
        self._cat_mode = None
        self._g_state_base = None
        self._dist_sampling = hip_config.get('dist_sampling', 'throughput')     # 'throughput' | 'parity' 
        self._dist_ready = False        # (collective decision, `_ready_to_train`)
        assert self._dist_sampling in ('throughput', 'parity')

        self._set_logger()

        if not use_replay_buffer:
            if self._dist is not None:
                raise ValueError('use_replay_buffer=False (the episode batch queue) is single-GPU: a data-parallel '
                                 "context (hip_config['dist']) is not supported with it")
            if self._lookahead:
                self._logger.info("hip_config['lookahead'] does not apply without a replay buffer: forced to 0")
                self._lookahead = 0

        if self.use_n_step_is and c_action_size == 0 and len(d_action_sizes) != 0 and discrete_dqn_like:
            self.use_n_step_is = False

        if device is None:
            if not torch.cuda.is_available():
                raise native.AsacNativeError('SAC_Base needs an MI355X (cuda/ROCm device); there is no CPU path')
            self.device = torch.device(f'cuda:{random.randint(0, torch.cuda.device_count() - 1)}')
        else:
            self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise native.AsacNativeError(f'SAC_Base needs a cuda/ROCm device, got {self.device}; no CPU fallback')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        native.load()
        self._logger.info(f'Device: {self.device.type}:{self.device.index}')

        if seed is not None:
            torch.manual_seed(seed)
            torch.cuda.manual_seed_all(seed)

        distributions.Distribution.set_default_validate_args(False)

        self.summary_writer = None
        self.summary_available = False
        if summary_path and self.model_abs_dir and self.train_mode and SummaryWriter is not None:
            self.summary_writer = SummaryWriter(str(Path(self.model_abs_dir).joinpath(summary_path)))
            self.summary_available = True

        self._profiler = UnifiedElapsedTimer(self._logger)
        self.noise = DeviceNoise()
        self._graph = None        # the train step's CapturedStep: the only holder of its graph's state
        self._graph_hp, self._all_optimizers = None, None     # `_optimizer_hp()` the captured graphs were made with
        self._graph_runs = {}     # run length -> _GraphRun
        self._la_graphs = {}      # hip_config['lookahead']: set parity -> CapturedStep
        self._graph_failed = False
        self._eager_steps = 0

        self._build_model(nn, nn_config, init_log_alpha, learning_rate)
        self._build_ckpt()
        self._init_replay_buffer(replay_config)
        self._init_or_restore(int(last_ckpt) if last_ckpt is not None else None)

    def _set_logger(self):
        self._logger = logging.getLogger('sac.base' if self.ma_name is None else f'sac.base.{self.ma_name}')

    # ==========================================================================================
    # construction (reference sac_base.py:271-491)
    # ==========================================================================================
    def _build_model(self, nn, nn_config, init_log_alpha, learning_rate) -> None:
        nn_config = defaultdict(dict, nn_config or {})
        rep_kw = nn_config['rep'] or {}
        pol_kw = nn_config['policy'] or {}
        dev = self.device

        self.global_step = torch.tensor(0, dtype=torch.int64, requires_grad=False, device='cpu')
        self._gamma_ratio = torch.logspace(0, self.n_step - 1, self.n_step, self.gamma, device=dev)
        self._lambda_ratio = torch.logspace(0, self.n_step - 1, self.n_step, self.v_lambda, device=dev)
        self._v_rho_f, self._v_c_f = float(self.v_rho), float(self.v_c)
        self.v_rho = torch.tensor(self.v_rho, device=dev)
        self.v_c = torch.tensor(self.v_c, device=dev)

        pad = [np.eye(s, dtype=np.float32)[0] for s in self.d_action_sizes]
        self._np_padding_action = np.concatenate(pad + [np.zeros(self.c_action_size, dtype=np.float32)], axis=-1)
        self._padding_action = torch.from_numpy(self._np_padding_action).to(dev)

        B = self.batch_size
        A_all = self.d_action_summed_size + self.c_action_size

        # -- representation ----------------------------------------------------------------------
        rep_args = (self.obs_names, self.obs_shapes, self.d_action_sizes, self.c_action_size)
        if fused_normalizer_applies(enabled=self._fused_normalizer, use_normalization=self.use_normalization,
                                    plain_learner=type(self)._plain_learner, data_parallel=self._dist is not None,
                                    float32_on_device=dev.type == 'cuda' and torch.get_default_dtype() == torch.float32):
            # the plugin's own class: every `type(...) is ModelSimpleRep` test sees what it sees without normalization; the
            # learner whitens in front of it (`_l_states_whitened` takes whitened observations, `get_l_states` raw ones)
            ModelRep = nn.ModelRep
            self.normalizer = Normalizer(self.obs_shapes, dev)
            self.normalizer_step = self.normalizer.normalizer_step
            self.running_means, self.running_variances = self.normalizer.running_means, self.normalizer.running_variances
        else:
            ModelRep = self._wrap_normalized_rep(nn.ModelRep) if self.use_normalization else nn.ModelRep
        self.model_rep = ModelRep(*rep_args, False, self.model_abs_dir, **rep_kw).to(dev)
        self.model_target_rep = ModelRep(*rep_args, True, self.model_abs_dir, **rep_kw).to(dev)
        if self._fuse_linear_tanh:     # the plugins' Linear + Tanh state heads: one launch per pass
            from .fused_linear import fuse_linear_tanh_heads
            fuse_linear_tanh_heads(self.model_rep), fuse_linear_tanh_heads(self.model_target_rep)
        test_obs = [torch.rand(B, 1, *s, device=dev) for s in self.obs_shapes]
        test_pre_action = torch.rand(B, 1, A_all, device=dev)
        test_rep_obs = test_obs if self.normalizer is None else self.normalizer.whiten(test_obs)
        with torch.no_grad():
            if self.seq_encoder == SEQ_ENCODER.ATTN:
                test_index = torch.zeros((B, 1), dtype=torch.int32, device=dev)
                st, hs, _ = self.model_rep(1, test_index, test_rep_obs, test_pre_action, None)
            else:
                st, hs = self.model_rep(test_rep_obs, test_pre_action, None)
        self.state_size, self.seq_hidden_state_shape = st.shape[-1], hs.shape[2:]
        for p in self.model_target_rep.parameters():
            p.requires_grad = False
        self._logger.info(f'State size: {self.state_size}')
        self._logger.info(f'Seq hidden state shape: {tuple(self.seq_hidden_state_shape)}')

        # -- Q ensemble and policy -----------------------------------------------------------------
        mk_q = lambda tgt: nn.ModelQ(self.state_size, self.d_action_sizes, self.c_action_size,  # noqa: E731
                                     tgt, self.model_abs_dir).to(dev)
        self.model_q_list = [mk_q(False) for _ in range(self.ensemble_q_num)]
        self.model_target_q_list = [mk_q(True) for _ in range(self.ensemble_q_num)]
        for q in self.model_target_q_list:
            for p in q.parameters():
                p.requires_grad = False
        self.model_policy = nn.ModelPolicy(self.state_size, self.d_action_sizes, self.c_action_size,
                                           self.model_abs_dir, **pol_kw).to(dev)

        # -- alpha -------------------------------------------------------------------------------------
        self.log_d_alpha = nn_parameter_scalar(init_log_alpha, dev)
        self.log_c_alpha = nn_parameter_scalar(init_log_alpha, dev)
        if self.d_action_sizes:
            sizes = torch.tensor(self.d_action_sizes, device=dev)
            sizes = torch.repeat_interleave(sizes.type(torch.float32), sizes)
            self.target_d_alpha = self.target_d_alpha * (-torch.log(1 / sizes))

        # -- curiosity -----------------------------------------------------------------------------------
        self.model_forward_dynamic = self.model_inverse_dynamic = None
        if self.curiosity == CURIOSITY.FORWARD:
            self.model_forward_dynamic = nn.ModelForwardDynamic(self.state_size, A_all).to(dev)
        elif self.curiosity == CURIOSITY.INVERSE:
            self.model_inverse_dynamic = nn.ModelInverseDynamic(self.state_size, A_all).to(dev)

        # -- flat parameter / gradient / moment buffers ------------------------------------------------------
        named = [('rep', list(self.model_rep.parameters()))]
        named += [(f'q_{i}', list(q.parameters())) for i, q in enumerate(self.model_q_list)]
        named += [('policy', list(self.model_policy.parameters())),
                  ('alpha', [self.log_d_alpha, self.log_c_alpha])]
        cur = self.model_forward_dynamic or self.model_inverse_dynamic
        if cur is not None:
            named.append(('curiosity', list(cur.parameters())))
        named += self._build_aux(nn, test_obs)      # siamese / prediction / RND heads (sac_aux.py)
        self._params = FlatParamGroup(named, dev, with_grad=True)
        tnamed = [('rep', list(self.model_target_rep.parameters()))]
        tnamed += [(f'q_{i}', list(q.parameters())) for i, q in enumerate(self.model_target_q_list)]
        self._target_params = FlatParamGroup(tnamed, dev, with_grad=False)
        self._polyak_len = self._params.span('rep', f'q_{self.ensemble_q_num - 1}')[1]
        assert self._polyak_len == self._target_params.numel
        if self._dist is not None:   # replicas start from rank 0's initialisation
            self._dist.broadcast_(self._params.flat)

        self._opt_steps = torch.zeros(1, dtype=torch.int64, device=dev)
        self._exp_avg = torch.zeros_like(self._params.flat)
        self._exp_avg_sq = torch.zeros_like(self._params.flat)

        def adam(names):
            if all(len(self._params.params[n]) == 0 for n in names):
                return None
            return FlatAdam(self._params, names, learning_rate, self._opt_steps, self._exp_avg, self._exp_avg_sq)

        self.optimizer_rep = adam(['rep'])
        self.optimizer_q_list = [adam([f'q_{i}']) for i in range(self.ensemble_q_num)]
        self.optimizer_policy = adam(['policy'])
        if self.use_auto_alpha:
            self.optimizer_alpha = adam(['alpha'])
        if cur is not None:
            self.optimizer_curiosity = adam(['curiosity'])
        if self.siamese is not None:
            self.optimizer_siamese = adam(['siamese'])
        if self.use_prediction:
            self.optimizer_prediction = adam(['prediction'])
        if self.use_rnd:
            self.optimizer_rnd = adam(['rnd'])

        # -- stock-network fast path: one MFMA launch per pass of the Q ensemble / policy ------------------------
        self._fq = self._ftq = self._fpi = None
        if self._use_fused_mlp and self.c_action_size and not self.d_action_sizes:
            dq = [describe_q(q) for q in self.model_q_list + self.model_target_q_list]
            seg = self._params.segments
            stride = seg['q_0'][1] - seg['q_0'][0]
            consecutive = all(seg[f'q_{i}'][0] == seg['q_0'][0] + i * stride for i in range(self.ensemble_q_num))
            if all(d is not None for d in dq) and consecutive:
                tseg = self._target_params.segments
                self._fq = StockMLP(dq[0], self._params.flat, self._params.grad, seg['q_0'][0], stride,
                                    self.ensemble_q_num, dev, [p for q in self.model_q_list for p in q.parameters()])
                self._ftq = StockMLP(dq[0], self._target_params.flat, None, tseg['q_0'][0], stride,
                                     self.ensemble_q_num, dev)
            dp = describe_policy(self.model_policy)
            if dp is not None:
                self._fpi = StockMLP(dp, self._params.flat, self._params.grad, seg['policy'][0],
                                     seg['policy'][1] - seg['policy'][0], 1, dev, list(self.model_policy.parameters()))
        self._attach_head_banks()
        self._wide_critics = self._fq is not None and self._fq.wide
        if self._wide_critics:
            # critics whose first layer is wider than 64 inputs (64-wide state + action): one launch per network pass — the
            # chains that pack several networks into one launch are not taken and no critic launch can host a sidecar job.
            # The jobs that do not need one still ride: the sampler in the step prologue, the write-backs' passes and the
            # temperature step in the TD error's return launch and the priority update (as after the fused policy chain)
            self._la_gather_sidecar = False
        self._logger.info(f'fused stock MLP path: Q={self._fq is not None} policy={self._fpi is not None}')
        # When the stock networks and the temperatures are the only trainable parameters, every gradient
        # slot is written exactly once per step by a kernel: overwrite instead of memset + accumulate.
        stock_only = {f'q_{i}' for i in range(self.ensemble_q_num)} | {'policy', 'alpha'}
        self._grads_overwrite = (self._fq is not None and self._fpi is not None and not self.offline_enabled
                                 and all(stop == start or name in stock_only
                                         for name, (start, stop) in self._params.segments.items()))
        if self._grads_overwrite:
            self._fq.accumulate = self._fpi.accumulate = False

        # -- static step buffers (stable addresses for graph replay) --------------------------------------------
        n, A, E, Es = self.n_step, self.c_action_size, self.ensemble_q_num, self.ensemble_q_sample
        f32 = dict(dtype=torch.float32, device=dev)
        A1 = max(A, 1)
        sizes = [B * (n + 1) * A1, B * A1, B * A1, B * (n + 1) * A1]     # consumption order of a step
        self._eps_all = torch.zeros(sum(sizes), **f32)
        o = np.cumsum([0] + sizes)
        self._eps_y = self._eps_all[o[0]:o[1]].view(B, n + 1, A1)
        self._eps_pi = self._eps_all[o[1]:o[2]].view(B, A1)
        self._eps_alpha = self._eps_all[o[2]:o[3]].view(B, A1)
        self._eps_td = self._eps_all[o[3]:o[4]].view(B, n + 1, A1)
        names = ('y_dn', 'y_dnext', 'y_cn', 'y_cnext', 'pi_d', 'pi_c', 'td_dn', 'td_dnext', 'td_cn', 'td_cnext')
        self._subsets_all = torch.arange(Es, dtype=torch.int32, device=dev).repeat(len(names), 1).contiguous()
        self._subsets = {k: self._subsets_all[i] for i, k in enumerate(names)}   # views of one buffer
        self._y_buf = torch.zeros(B, **f32)
        self._y_td_buf = torch.zeros(B, **f32)
        self._td_error = torch.zeros(B, **f32)
        self._stats = {k: torch.zeros((), **f32) for k in ('d_entropy', 'c_entropy', 'loss_curiosity', 'loss_policy')}
        self._loss_q_e = torch.zeros(E, **f32)             # per-ensemble Q losses of the last step
        self._stats['loss_q'] = self._loss_q_e[0]
        self._grad_q = torch.zeros(E, B, **f32)            # d loss / d q written by the loss kernels
        # zeroed exchange words of `asac_mse_mean_grad` (the observation model's frame loss, sac_aux._train_rpm)
        self._mse_big_ws = torch.zeros(native.mse_mean_grad_workspace(), **f32) if self.use_prediction else None
        self._grad_logp = torch.zeros(B, **f32)
        # pure-discrete learner (`_discrete_fused`): the branch table and d loss / d (head outputs) of its two loss launches
        self._branches = native.branches(self.d_action_sizes) if self.d_action_sizes else None
        self._discrete_grads = {}       # batch rows -> (d loss_q / d q [E, B, D], d loss_policy / d logits [B, D])
        # hybrid learner (`_hybrid_fused`): batch rows -> the discrete returns' targets (the continuous ones go to `_y_buf` /
        # `_y_td_buf`) and the gradients its two loss launches write
        self._hybrid_bufs = {}
        # the one hand-over between steps that goes through `self`, from the Q step's return target to the policy step
        # (`_train_policy` has the reference's signature: no room for either): `_ls_y` = the policy's output over the
        # return's window, read by `_step_policy`; `_pi_sampled` = the return's sampling launch also drew the policy
        # step's action at t = 0 into `_pi_a` / `_pi_logp`, taken and cleared by `_train_policy_stock`; `_pi_saved` = the
        # Q-loss backward launch also ran the policy's forward on the policy step's rows as a rider: (save buffer, data
        # pointer, row stride, N of those rows), set or cleared by every `_stock_q_backward`, taken and cleared by
        # `_train_policy_stock`, which loads the forward only for exactly those rows and the action `_pi_sampled` hands it
        self._ls_y = None
        self._pi_saved = None
        self._rider_plan_cache = None   # (rows and return it was decided for, the save buffer or None): `_rider_plan`
        self._critic_plan_cache = {}    # stored pair and window (a static set) -> the save buffer or None: `_critic_rider_plan`
        self._cq_buf, self._tq_buf, self._cq_td_buf = (torch.zeros(E, B, 1, **f32) for _ in range(3))
        self._pi_q, self._pi_stats_src = torch.zeros(E, B, 1, **f32), None
        self._pi_a, self._pi_logp, self._pi_sampled = torch.zeros(B, A1, **f32), torch.zeros(B, **f32), False
        # online + target representation over the same window: fused GRU layers pair up in one launch
        self._rep_twin = None
        if self._twin_rep and type(self.model_rep) is not ModelSimpleRep:
            from .fused_gru import TwinPass
            self._rep_twin = TwinPass(self.model_rep, self.model_target_rep)

    def _build_ckpt(self) -> None:
        """name -> module / optimizer / tensor, same keys as the reference (sac_base.py:493-566)."""
        ck = self.ckpt_dict = {'global_step': self.global_step}
        if self.optimizer_rep is not None:
            ck['model_rep'], ck['model_target_rep'], ck['optimizer_rep'] = \
                self.model_rep, self.model_target_rep, self.optimizer_rep
        for i in range(self.ensemble_q_num):
            ck[f'model_q_{i}'] = self.model_q_list[i]
            ck[f'model_target_q_{i}'] = self.model_target_q_list[i]
            ck[f'optimizer_q_{i}'] = self.optimizer_q_list[i]
        ck['model_policy'], ck['optimizer_policy'] = self.model_policy, self.optimizer_policy
        ck['log_d_alpha'], ck['log_c_alpha'] = self.log_d_alpha, self.log_c_alpha
        if self.use_auto_alpha:
            ck['optimizer_alpha'] = self.optimizer_alpha
        if self.curiosity == CURIOSITY.FORWARD:
            ck['model_forward_dynamic'] = self.model_forward_dynamic
        elif self.curiosity == CURIOSITY.INVERSE:
            ck['model_inverse_dynamic'] = self.model_inverse_dynamic
        if self.curiosity is not None:
            ck['optimizer_curiosity'] = self.optimizer_curiosity
        self._aux_ckpt(ck)
        total = sum(p.numel() for m in ck.values() if isinstance(m, nn.Module) for p in m.parameters())
        self._logger.info(f'Parameters: {total}')

    def _init_or_restore(self, last_ckpt: int | None) -> None:
        """sac_base.py:568-629."""
        self.ckpt_dir = None
        if not self.model_abs_dir:
            self._update_target_variables()
            return
        self.ckpt_dir = ckpt_dir = Path(self.model_abs_dir).joinpath('model')
        ckpts = sorted(int(p.stem) for p in ckpt_dir.glob('*.pth')) if ckpt_dir.exists() else []
        ckpt_dir.mkdir(parents=True, exist_ok=True)
        if not ckpts:
            self._logger.info('Initializing from scratch')
            self._update_target_variables()
            return
        if last_ckpt is None or last_ckpt not in ckpts:
            if last_ckpt is not None:
                self._logger.warning(f'{last_ckpt} NOT IN {ckpts}, using {ckpts[-1]}')
            last_ckpt = ckpts[-1]
        path = ckpt_dir.joinpath(f'{last_ckpt}.pth')
        restored = torch.load(path, map_location=self.device, weights_only=True)
        failed = False
        for name, obj in self.ckpt_dict.items():
            if name not in restored:
                self._logger.warning(f'{name} not in {last_ckpt}.pth')
                continue
            if isinstance(obj, torch.Tensor):
                if name == 'global_step':
                    self.global_step.copy_(restored[name].to('cpu'))
                else:
                    with torch.no_grad():
                        obj.copy_(restored[name])
                continue
            try:
                if failed and name.startswith('optimizer'):
                    continue
                obj.load_state_dict(restored[name])
            except RuntimeError as e:
                failed = True
                self._logger.error(e)
            if isinstance(obj, nn.Module):
                obj.train(self.train_mode)
        self._params.rebind()
        self._target_params.rebind()
        self._logger.info(f'Restored from {path}')
        if self.train_mode and self.use_replay_buffer:
            self.replay_buffer.load(ckpt_dir, last_ckpt)
            self._logger.info('Replay buffer restored')

    def _init_replay_buffer(self, replay_config: dict | None = None) -> None:
        if not self.train_mode:
            return
        if not self.use_replay_buffer:
            # (reference sac_base.py:640-644; the windows' padding action is the learner's)
            self.batch_buffer = BatchBuffer(burn_in_step=self.burn_in_step,
                                            n_step=self.n_step,
                                            padding_action=self._padding_action,
                                            batch_size=self.batch_size,
                                            device=self.device,
                                            obs_names=self.obs_names)
            return
        self.replay_buffer = PrioritizedReplayBuffer(batch_size=self.batch_size,
                                                     sample_prev_n=self.burn_in_step,
                                                     sample_post_n=self.n_step,
                                                     device=self.device,
                                                     logger_parent_name=self._logger.name,
                                                     **(replay_config or {}))
        self.replay_buffer.set_window_padding(self._padding_action)
        self.replay_buffer.uniform_source = self.noise
        self._cat_mode = None
        if self._adjacent_cat and type(self.model_rep) is not ModelSimpleRep:
            # a user representation receives (obs, previous actions): keep them side by side in the static batch so
            # that the concatenation sequence modules start with is a view (adjacent_cat.py); the gather then also
            # delivers the derived window inputs (index_x, padding_mask_x, pre_action) in its own launch
            from .adjacent_cat import AdjacentCat
            self.replay_buffer.join_vector_obs_with_pre_action(self.d_action_summed_size + self.c_action_size)
            width = native.LINEAR_TANH_MAX_IN if (self._deferred_cat and self._fuse_linear_tanh) else 0
            # (deferred only at the widths a fused head of this representation takes: nothing else can use the two blocks)
            from .fused_linear import LinearTanhHead
            widths = {m[0].in_features for m in self.model_rep.modules() if isinstance(m, LinearTanhHead)}
            self._cat_mode = lambda: AdjacentCat(width if widths else 0, widths)
        if self._dist is not None and self._dist_sampling == 'parity':
            # SURVEY 8e "parity": every batch is the reference's stratified sample over the UNION of the ranks' shards
            # (global batch = world_size * batch_size, this rank trains on batch_size rows of it)
            from .parallel import ProductShard, ShardedParityReplay
            rb = self.replay_buffer
            global_batch = self.batch_size * self._dist.world_size
            rb.sharded = ShardedParityReplay(self._dist, ProductShard(rb, global_batch), global_batch, self.device)
            rb._u = torch.zeros(global_batch, dtype=torch.float64, device=self.device)    # the GLOBAL batch's uniforms
        elif self._dist is not None:
            self.replay_buffer.min_ratio_reducer = self._dist.all_reduce_min_

    # ==========================================================================================
    # small public surface (reference sac_base.py:648-743)
    # ==========================================================================================
    def set_train_mode(self, train_mode=True):
        self.train_mode = train_mode
        for m in self.ckpt_dict.values():
            if isinstance(m, nn.Module):
                m.train(mode=train_mode)

    def save_model(self, save_replay_buffer=False) -> None:
        if self.ckpt_dir is None:
            return
        if self.use_replay_buffer and self.train_mode:
            self.replay_buffer.check_health()      # never write a checkpoint of a run whose td-errors went NaN
        step = self.get_global_step()
        path = self.ckpt_dir.joinpath(f'{step}.pth')
        torch.save({k: (v.detach().clone() if isinstance(v, torch.Tensor) else v.state_dict())
                    for k, v in self.ckpt_dict.items()}, path)
        self._logger.info(f'Model saved at {path}')
        if self.use_replay_buffer and save_replay_buffer:
            self.replay_buffer.save(self.ckpt_dir, step)

    def write_constant_summaries(self, constant_summaries: list[dict], iteration=None) -> None:
        if self.summary_writer is None:
            return
        for s in constant_summaries:
            self.summary_writer.add_scalar(s['tag'], s['simple_value'],
                                           self.get_global_step() if iteration is None else iteration)
        self.summary_writer.flush()

    def write_histogram_summaries(self, histograms, iteration=None) -> None:
        if self.summary_writer is None:
            return
        for s in histograms:
            self.summary_writer.add_histogram(s['tag'], s['histogram'],
                                              self.get_global_step() if iteration is None else iteration)
        self.summary_writer.flush()

    def log_episode(self, force: bool = False, **episode_trans) -> None:
        if not force and (self.summary_writer is None or not self.summary_available):
            return
        self.summary_available = False

    def increase_global_step(self) -> int:
        self.global_step.add_(1)
        return self.global_step.item()

    def set_global_step(self, global_step):
        if isinstance(global_step, torch.Tensor):
            global_step = global_step.item()
        if global_step == self.get_global_step():
            return
        self._logger.warning(f'Global step {self.get_global_step()} -> {global_step}')
        self.global_step.fill_(global_step)

    def get_global_step(self) -> int:
        return self.global_step.item()

    def get_initial_action(self, batch_size, get_numpy=True):
        if get_numpy:
            parts = [np.eye(s, dtype=np.float32)[np.random.randint(0, s, size=batch_size)]
                     for s in self.d_action_sizes]
            parts.append(np.zeros([batch_size, self.c_action_size], dtype=np.float32))
            return np.concatenate(parts, axis=-1)
        parts = [functional.one_hot(torch.randint(0, s, (batch_size,), device=self.device), num_classes=s).float()
                 for s in self.d_action_sizes]
        parts.append(torch.zeros((batch_size, self.c_action_size), device=self.device))
        return torch.cat(parts, dim=-1)

    def get_initial_seq_hidden_state(self, batch_size, get_numpy=True):
        if get_numpy:
            return np.zeros([batch_size, *self.seq_hidden_state_shape], dtype=np.float32)
        return torch.zeros([batch_size, *self.seq_hidden_state_shape], device=self.device)

    @torch.no_grad()
    def _update_target_variables(self, tau=1.) -> None:
        """Polyak over the flat [rep | q_0 .. q_E-1] buffers: one launch (reference 745-764 loops
        over parameters with three kernels each)."""
        if self._polyak_len > 0:
            native.polyak(self._target_params.flat[:self._polyak_len], self._params.flat[:self._polyak_len], tau)

    def _process_torch_obs_list(self, obs_list):
        for i, o in enumerate(obs_list):
            if o.dtype == torch.uint8:
                obs_list[i] = o.type(torch.float32) / 255.
            elif o.dtype == torch.bool:
                obs_list[i] = o.type(torch.float32)

    # ==========================================================================================
    # acting (reference sac_base.py:858-1086) — eager torch, NumPy in/out, not on the train path
    # ==========================================================================================
    @torch.no_grad()
    def _random_action(self, d_action, c_action):
        if self.action_noise is None:
            return d_action, c_action
        batch = max(d_action.shape[0], c_action.shape[0])
        noise = torch.linspace(*self.action_noise, steps=batch, device=self.device)
        if self.d_action_sizes:
            rnd = [functional.one_hot(torch.argmax(torch.rand(batch, s, device=self.device), dim=-1), s)
                   for s in self.d_action_sizes]
            rnd = torch.cat(rnd, dim=-1).type(torch.float32)
            mask = torch.rand(batch, device=self.device) < noise
            d_action[mask] = rnd[mask]
        if self.c_action_size:
            c_action = torch.tanh(torch.atanh(c_action)
                                  + torch.randn(batch, self.c_action_size, device=self.device) * noise.unsqueeze(1))
        return d_action, c_action

    @torch.no_grad()
    def _choose_action(self, obs_list, state, offline_action=None, disable_sample=False,
                       force_rnd_if_available=False):
        batch = state.shape[0]
        use_rnd = self.use_rnd and (self.train_mode or force_rnd_if_available)
        if (offline_action is None and not use_rnd and self.action_noise is None and self._stock_c_only()
                and state.dim() == 2):
            # stock Gaussian policy, continuous actions only: the policy's forward is ONE launch (`asac_mlp_forward`),
            # the sample and the probability of the chosen action one elementwise launch each — instead of ~25 eager
            # module / distribution launches (0.45 ms of host time per environment step)
            A = self.c_action_size
            ls = self._fpi._launch_forward(StockMLP._rows(state, self.state_size), None)[0]      # [batch, 2A] (loc | scale)
            loc, scale = ls[:, :A], ls[:, A:]
            if disable_sample:
                c_action = torch.tanh(loc)
            else:
                eps = torch.empty((batch, A), dtype=torch.float32, device=self.device)
                self.noise.normal_(eps)
                c_action = torch.empty((batch, A), dtype=torch.float32, device=self.device)
                native.squash_sample_fwd(loc, scale, eps, c_action, torch.empty(batch, dtype=torch.float32, device=self.device))
            prob = torch.empty((batch, A), dtype=torch.float32, device=self.device)
            win = lambda t: t.as_strided((batch, 1, A), (t.stride(0), t.stride(0), 1))  # noqa: E731
            native.squash_prob(win(loc), win(scale), win(c_action), 0, win(prob), 0)
            return c_action, prob
        if (use_rnd and offline_action is None and not disable_sample and self.action_noise is None and self._stock_c_only()
                and state.dim() == 2 and (rnd := self._rnd_fused(rows=batch * self.rnd_n_sample)) is not None):
            # novelty-guided acting on the stock networks: the policy's forward, the Gaussian draws of the rnd_n_sample
            # candidates, then ONE launch for the candidates, both RND stacks on them, the first largest distillation error
            # per entry and the chosen action's probability — instead of the policy module, `Normal.sample`, two
            # concatenations, four ResBlocks, pow / sum / argmax, an index and `squash_correction_prob` per environment step
            A, k = self.c_action_size, self.rnd_n_sample
            ls = self._fpi._launch_forward(StockMLP._rows(state, self.state_size), None)[0]      # [batch, 2A] (loc | scale)
            eps = torch.empty((batch, k, A), dtype=torch.float32, device=self.device)
            self.noise.normal_(eps)
            c_action = torch.empty((batch, A), dtype=torch.float32, device=self.device)
            prob = torch.empty((batch, A), dtype=torch.float32, device=self.device)
            native.rnd_pick(rnd[0], rnd[1], rnd[2], StockMLP._rows(state, self.state_size), ls[:, :A], ls[:, A:], eps,
                            c_action, prob)
            return c_action, prob
        if (use_rnd and offline_action is None and not disable_sample and self.action_noise is None and state.dim() == 2
                and (drnd := self._drnd_fused(rows=batch * self.rnd_n_sample)) is not None):
            # novelty-guided acting, discrete branches with a policy: the policy's logits (`_discrete_logits`: the stock
            # policy's raw head outputs, the distribution logits of a plugin policy that has its own `forward`), the
            # uniforms of the rnd_n_sample candidates, then ONE launch for the branch softmax, the candidates (inverse CDF),
            # both stacks of all D members of `d_dense_list`, the first largest distillation error per entry and the
            # one-hot action — instead of 2 D two-block stacks, two `torch.stack`, `OneHotCategorical.sample((k,))` per
            # branch, two [batch, k, D, 64] broadcast products and pow / sum / argmax / index per environment step
            D = self.d_action_summed_size
            logits = self._discrete_logits(state, obs_list)
            u = torch.empty((batch, self.rnd_n_sample, self.d_action_branch_size), dtype=torch.float32, device=self.device)
            self.noise.uniform_(u)
            d_action = torch.empty((batch, D), dtype=torch.float32, device=self.device)
            prob = torch.empty((batch, D), dtype=torch.float32, device=self.device)
            native.drnd_pick(self._branches, drnd[0], drnd[1], drnd[2], StockMLP._rows(state, self.state_size), logits, u,
                             d_action, prob)
            return d_action, prob
        if offline_action is None and not use_rnd and state.dim() == 2 and self._dqn_fused(1, acting=True):
            # DQN-like, discrete branches only: the first critic's forward, then ONE launch for the greedy one-hot per
            # branch and (train mode) the epsilon-random rows, their uniforms drawn on the device — instead of ~30 eager
            # launches and a host-to-device copy of the mask per environment step.  The policy is not evaluated: nothing
            # of it is read (`prob` is ones).
            d_qs, _ = self.model_q_list[0](state, None, obs_list)
            d_action = torch.empty((batch, self.d_action_summed_size), dtype=torch.float32, device=self.device)
            u = None
            if self.train_mode:
                u = torch.empty((batch, 1 + self.d_action_branch_size), dtype=torch.float32, device=self.device)
                self.noise.uniform_(u)
            native.dqn_act(self._branches, d_qs, u, self.discrete_dqn_epsilon, d_action)
            d_action, _ = self._random_action(d_action, torch.zeros(0, device=self.device))
            return d_action, torch.ones((batch, self.d_action_summed_size), device=self.device)
        if fused_act_applies(
                enabled=self._fused_act, plain_learner=type(self)._plain_learner, d_action_sizes=self.d_action_sizes,
                c_action_size=self.c_action_size, discrete_dqn_like=bool(self.d_action_sizes) and self.discrete_dqn_like,
                rnd_in_effect=use_rnd, offline_action=offline_action is not None,
                float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
                state_dim=state.dim()):
            # every other policy-based case — discrete branches, hybrid spaces, `action_noise`, `disable_sample`, a plugin
            # policy: the policy's head outputs (the stock policy's raw heads, the distribution parameters of a policy that
            # has its own `forward`), at most one uniform and one Gaussian draw buffer, then ONE launch for the branch
            # softmax, the sampled / greatest / noise-random one-hots, the squashed Gaussian action, its noise and the
            # probabilities — instead of the distribution objects, `OneHotCategorical.sample()` per branch,
            # `_random_action` and the ones / slice / `squash_correction_prob` / concatenation tail below
            K, D, A = self.d_action_branch_size, self.d_action_summed_size, self.c_action_size
            f32 = dict(dtype=torch.float32, device=self.device)
            logits = loc = scale = None
            stock = type(self.model_policy).forward is ModelPolicy.forward
            if stock and self._stock_c_only():       # (`action_noise`: the fused forward's [batch, 2A] (loc | scale) rows)
                ls = self._fpi._launch_forward(StockMLP._rows(state, self.state_size), None)[0]
                loc, scale, stock = ls[:, :A], ls[:, A:], False
            elif stock:
                logits, loc, scale = self.model_policy.heads_raw(state)
            else:
                d_policy, c_policy = self.model_policy(state, obs_list)
                if D:
                    logits = d_policy.logits
                if A:
                    loc, scale = c_policy.loc.contiguous(), c_policy.scale.contiguous()
            nu, ne = native.act_draw_columns(K, A, bool(disable_sample), self.action_noise is not None)
            u = eps = None
            if nu:
                u = torch.empty((batch, nu), **f32)
                self.noise.uniform_(u)
            if ne:
                eps = torch.empty((batch, ne), **f32)
                self.noise.normal_(eps)
            action, prob = torch.empty((batch, D + A), **f32), torch.empty((batch, D + A), **f32)
            native.act_policy(native.act_job(self._branches, logits, loc, scale, u, eps, action, prob, head_raw=stock,
                                             deterministic=disable_sample, action_noise=self.action_noise))
            return action, prob
        d_policy, c_policy = self.model_policy(state, obs_list)
        if offline_action is None:
            if self.d_action_sizes and self.discrete_dqn_like:
                # greedy w.r.t. the first critic, epsilon / RND-novelty random (reference 904-930)
                d_qs, _ = self.model_q_list[0](state, c_policy.sample() if self.c_action_size else None, obs_list)
                d_action = torch.cat([functional.one_hot(torch.argmax(part, dim=-1), size).type(torch.float32)
                                      for part, size in zip(d_qs.split(self.d_action_sizes, dim=-1),
                                                            self.d_action_sizes)], dim=-1)
                if self.train_mode:
                    if use_rnd:
                        s_rnd = torch.sigmoid(self.model_rnd.cal_s_rnd(state))
                        t_rnd = torch.sigmoid(self.model_target_rnd.cal_s_rnd(state))
                        mask = torch.rand(batch).to(self.device) < torch.mean(torch.abs(s_rnd - t_rnd), dim=-1)
                    else:
                        mask = (torch.rand(batch) < self.discrete_dqn_epsilon).to(self.device)
                    rnd_d = torch.cat([distributions.OneHotCategorical(
                        logits=torch.ones((batch, size), device=self.device), validate_args=False).sample()
                        for size in self.d_action_sizes], dim=-1)
                    d_action[mask] = rnd_d[mask]
            elif self.d_action_sizes:
                if disable_sample:
                    d_action = d_policy.sample_deter()
                elif use_rnd:
                    d_action = self.rnd_sample_d_action(state, d_policy)
                else:
                    d_action = d_policy.sample()
                d_action = d_action.type(torch.float32)
            else:
                d_action = torch.zeros(0, device=self.device)
            if self.c_action_size:
                if disable_sample:
                    c_action = torch.tanh(c_policy.mean)
                elif use_rnd:
                    c_action = self.rnd_sample_c_action(state, c_policy)
                else:   # `c_policy.sample()` (reference 944) with the Gaussian draw taken from `self.noise`
                    eps = torch.empty_like(c_policy.loc)
                    self.noise.normal_(eps)
                    c_action = torch.tanh(self._rsample(c_policy, eps))
            else:
                c_action = torch.zeros(0, device=self.device)
            d_action, c_action = self._random_action(d_action, c_action)
        else:
            d_action = offline_action[..., :self.d_action_summed_size]
            c_action = offline_action[..., self.d_action_summed_size:]
        prob = torch.ones((batch, self.d_action_summed_size + self.c_action_size), device=self.device)
        if self.d_action_sizes and not self.discrete_dqn_like:
            prob[:, :self.d_action_summed_size] = d_policy.probs
        if self.c_action_size:
            prob[:, self.d_action_summed_size:] = squash_correction_prob(
                c_policy, torch.atanh(torch.clamp(c_action, -0.999, 0.999)))
        if not self.d_action_sizes:
            return c_action, prob
        if not self.c_action_size:
            return d_action, prob
        return torch.cat([d_action, c_action], dim=-1), prob

    @torch.no_grad()
    def choose_action_device(self, obs_list, pre_action, pre_seq_hidden_state, offline_action=None,
                             disable_sample=False, force_rnd_if_available=False):
        """`choose_action` on tensors that already live in HBM (the device-resident `AgentManager`,
        algorithm/agent.py): same computation, no host round trip; returns device tensors."""
        obs_list = list(obs_list)
        self._process_torch_obs_list(obs_list)
        rep_obs = obs_list if self.normalizer is None else self.normalizer.whiten(obs_list)
        state, next_hidden = self.model_rep([o.unsqueeze(1) for o in rep_obs], pre_action.unsqueeze(1),
                                            pre_seq_hidden_state.unsqueeze(1))
        action, prob = self._choose_action(obs_list, state.squeeze(1), offline_action, disable_sample,
                                           force_rnd_if_available)
        return action, prob, next_hidden.squeeze(1)

    @torch.no_grad()
    def choose_action(self, obs_list, pre_action, pre_seq_hidden_state, offline_action=None,
                      disable_sample=False, force_rnd_if_available=False):
        dev = lambda x: torch.from_numpy(x).to(self.device)  # noqa: E731
        action, prob, next_hidden = self.choose_action_device(
            [dev(o) for o in obs_list], dev(pre_action), dev(pre_seq_hidden_state),
            dev(offline_action) if offline_action is not None else None, disable_sample, force_rnd_if_available)
        return action.cpu().numpy(), prob.cpu().numpy(), next_hidden.cpu().numpy()

    @torch.no_grad()
    def choose_attn_action_device(self, ep_indexes, ep_padding_masks, ep_obses_list, ep_pre_actions,
                                  ep_pre_attn_states, offline_action=None, disable_sample=False,
                                  force_rnd_if_available=False):
        """`choose_attn_action` on device tensors (windows of at most `burn_in_step` positions, which is all the
        reference keeps of what it is handed, sac_base.py:1049-1053); returns device tensors."""
        w = self.burn_in_step
        cut = lambda x: x[:, -w:]  # noqa: E731
        obs = [cut(o) for o in ep_obses_list]
        self._process_torch_obs_list(obs)
        rep_obs = obs if self.normalizer is None else self.normalizer.whiten(obs)
        state, attn_state, _ = self.model_rep(1, cut(ep_indexes), rep_obs, cut(ep_pre_actions),
                                              pre_seq_hidden_state=cut(ep_pre_attn_states),
                                              is_prev_hidden_state=False, padding_mask=cut(ep_padding_masks))
        action, prob = self._choose_action([o[:, -1] for o in obs], state.squeeze(1), offline_action,
                                           disable_sample, force_rnd_if_available)
        return action, prob, attn_state.squeeze(1)

    @torch.no_grad()
    def choose_attn_action(self, ep_indexes, ep_padding_masks, ep_obses_list, ep_pre_actions,
                           ep_pre_attn_states, offline_action=None, disable_sample=False,
                           force_rnd_if_available=False):
        w = self.burn_in_step
        to = lambda x: torch.from_numpy(x[:, -w:]).to(self.device)  # noqa: E731
        action, prob, attn_state = self.choose_attn_action_device(
            to(ep_indexes), to(ep_padding_masks), [to(o) for o in ep_obses_list], to(ep_pre_actions),
            to(ep_pre_attn_states),
            torch.from_numpy(offline_action).to(self.device) if offline_action is not None else None,
            disable_sample, force_rnd_if_available)
        return action.cpu().numpy(), prob.cpu().numpy(), attn_state.cpu().numpy()

    # ==========================================================================================
    # states (reference sac_base.py:1090-1189)
    # ==========================================================================================
    def get_bnx_data(self, bn_indexes, bn_padding_masks, bn_actions, pre_action_out=None):
        if (bn_indexes.is_cuda and bn_indexes.dtype == torch.int32 and bn_indexes.shape[1] >= 1
                and bn_padding_masks.dtype == torch.bool and bn_actions.dtype == torch.float32
                and bn_indexes.stride(1) == 1 and bn_padding_masks.stride(1) == 1 and bn_actions.stride(2) == 1):
            B, Lm1 = bn_indexes.shape      # one launch instead of six concatenation / fill kernels
            index_x = torch.empty((B, Lm1 + 1), dtype=torch.int32, device=bn_indexes.device)
            pad_x = torch.empty((B, Lm1 + 1), dtype=torch.bool, device=bn_indexes.device)
            pre_action = pre_action_out      # (the static batch's column block beside the vector observations)
            if pre_action is None or pre_action.shape != (B, Lm1 + 1, bn_actions.shape[-1]):
                pre_action = torch.empty((B, Lm1 + 1, bn_actions.shape[-1]), dtype=torch.float32, device=bn_indexes.device)
            native.window_aux(bn_indexes, bn_padding_masks, bn_actions, index_x, pad_x, pre_action)
            return index_x, pad_x, pre_action
        bnx_indexes = torch.concat([bn_indexes, bn_indexes[:, -1:] + (bn_indexes[:, -1:] != -1)], dim=1)
        bnx_padding_masks = torch.concat([bn_padding_masks, bn_padding_masks[:, -1:]], dim=1)
        return bnx_indexes, bnx_padding_masks, gen_n_pre_actions(bn_actions, keep_last_action=True)

    def whiten_obs(self, obs_list):
        """`obs_list` as `model_rep.forward` expects it: whitened by the running statistics under
        `hip_config['fused_normalizer']` (for callers that use `model_rep` directly), else unchanged — a `NormalizedRep`
        whitens inside its forward"""
        return list(obs_list) if self.normalizer is None else self.normalizer.whiten(obs_list)

    def get_l_states(self, l_indexes, l_padding_masks, l_obses_list, l_pre_actions, l_pre_seq_hidden_states,
                     is_target=False):
        """The reference's contract: RAW observations in, whatever normalizes them."""
        if self.normalizer is not None:
            l_obses_list = self.normalizer.whiten(l_obses_list)
        return self._l_states_whitened(l_indexes, l_padding_masks, l_obses_list, l_pre_actions, l_pre_seq_hidden_states,
                                       is_target=is_target)

    def _l_states_whitened(self, l_indexes, l_padding_masks, l_obses_list, l_pre_actions, l_pre_seq_hidden_states,
                           is_target=False):
        """`get_l_states` on observations the representation takes as they are: the step's own passes over `w.rep_in`,
        whitened once a step by `_window_views`"""
        rep = self.model_target_rep if is_target else self.model_rep
        if self.seq_encoder == SEQ_ENCODER.ATTN:
            st, attn, _ = rep(l_indexes.shape[1], l_indexes, l_obses_list, l_pre_actions,
                              l_pre_seq_hidden_states[:, :1], is_prev_hidden_state=True,
                              padding_mask=l_padding_masks)
            return _real(st), _real(attn)
        out = rep(l_obses_list, l_pre_actions, l_pre_seq_hidden_states, padding_mask=l_padding_masks)
        return tuple(_real(o) for o in out) if isinstance(out, tuple) else _real(out)

    # ------------------------------------------------------------------------------------------
    # network evaluation: fused stock path or the user modules
    # ------------------------------------------------------------------------------------------
    def _c_q_values(self, target: bool, state, c_action, obs_list, param_grads=True, select=None):
        """Continuous Q of every ensemble member -> [E, *state.shape[:-1]].  `select` = (window [B, L, S], t)
        when `state` is `window[:, t]`: lets the fused path differentiate into the window directly."""
        fused = self._ftq if target else self._fq
        if fused is not None:
            lead = state.shape[:-1]
            a_rows = StockMLP._rows(c_action, self.c_action_size)
            if select is not None and not target and select[0].dim() == 3 and select[0].is_contiguous():
                out = fused.call_select(select[0], select[1], a_rows, param_grads=param_grads)
            else:
                rows = StockMLP._rows if torch.is_grad_enabled() else StockMLP._rows_in_place
                out = fused(rows(state, self.state_size), a_rows, param_grads=param_grads and not target)
            return out.view(self.ensemble_q_num, *lead)
        models = self.model_target_q_list if target else self.model_q_list
        return torch.stack([q(state, c_action, obs_list)[1] for q in models]).squeeze(-1)

    def _policy(self, state, obs_list):
        """-> (d_policy, c_policy, loc, scale, plain): `plain` says (loc, scale) fully describe the
        continuous head (torch Normal or the fused stock policy), so the fused squash kernels apply;
        c_policy is None on the fused path."""
        if self._fpi is not None:
            lead, A = state.shape[:-1], self.c_action_size
            rows = StockMLP._rows if torch.is_grad_enabled() else StockMLP._rows_in_place
            self._ls = self._fpi(rows(state, self.state_size))[0].view(*lead, 2 * A)   # (loc | scale)
            return None, None, self._ls[..., :A], self._ls[..., A:], True
        self._ls = None
        d_policy, c_policy = self.model_policy(state, obs_list)
        if c_policy is None:
            return d_policy, None, None, None, False
        plain = type(c_policy) is distributions.Normal
        return d_policy, c_policy, c_policy.loc, c_policy.scale, plain

    @staticmethod
    def _rsample(c_policy, eps):
        """reference `Normal.rsample` / `NormalWithPadding.rsample` with externally drawn noise"""
        if hasattr(c_policy, 'padding_mask'):
            keep = ~c_policy.padding_mask
            return c_policy.loc * keep + eps * (c_policy.scale * keep)
        return c_policy.loc + eps * c_policy.scale

    @torch.no_grad()
    def get_l_probs(self, l_obses_list, l_states, l_actions):
        """pi-probability of the stored actions over the window (new mu for the next visit)."""
        d_policy, c_policy, loc, scale, plain = self._policy(l_states, l_obses_list)
        A_all = self.d_action_summed_size + self.c_action_size
        probs = torch.empty((*l_states.shape[:2], A_all), dtype=torch.float32, device=self.device)
        if self.d_action_sizes:
            probs[..., :self.d_action_summed_size] = d_policy.probs
        if self.c_action_size:
            if plain and l_actions.stride(-1) == 1:
                native.squash_prob(loc, scale, l_actions, self.d_action_summed_size, probs,
                                   self.d_action_summed_size)
            else:
                c_act = l_actions[..., self.d_action_summed_size:]
                probs[..., self.d_action_summed_size:] = squash_correction_prob(
                    c_policy, torch.atanh(torch.clamp(c_act, -0.999, 0.999)))
        return probs

    def _return_sample_epilogue(self, jobs, k, ls, nx_actions, eps_buf, policy_sample):
        """What `_get_y` does with the policy's output over `nx_states` right after the forward — rsample / tanh / log-prob,
        pi(stored actions) under `use_n_step_is`, with `policy_sample` the policy step's draw at t = 0 (reference
        sac_base.py:1346-1351, 1430, 1452) — as the EPILOGUE of that forward's launch (`jobs[k]` of
        `native.mlp_forward_multi_sampled`: no elementwise launch behind it).  Where the form applies the step's noise is
        drawn as `_get_y` would have and the launch is issued;  -> ((a_tanh, logp), c_pi) to hand to
        `_get_y(sample=, stored_pi=)`, or None: nothing drawn, nothing launched."""
        A = self.c_action_size
        if not (native.SAMPLE_EPILOGUE and A and 2 * A <= 16 and ls.dim() == 3 and nx_actions.stride(-1) == 1):
            return None
        f32 = dict(dtype=torch.float32, device=self.device)
        a_tanh, logp = torch.empty((*ls.shape[:2], A), **f32), torch.empty(ls.shape[:2], **f32)
        c_pi = torch.empty((*ls.shape[:2], A), **f32) if self.use_n_step_is else None
        epis = [native.sample_epilogue() for _ in jobs]
        epis[k] = native.sample_epilogue(jobs[k], eps_buf, a_tanh, logp, ls.shape[1],
                                         action=nx_actions if self.use_n_step_is else None,
                                         action_offset=self.d_action_summed_size, prob_out=c_pi,
                                         eps2=self._eps_pi if policy_sample else None, t2=0,
                                         a2_out=self._pi_a if policy_sample else None,
                                         logp2_out=self._pi_logp if policy_sample else None)
        if not native.mlp_forward_multi_sampled_ok(jobs, epis):
            return None
        self.noise.normal_(eps_buf)
        if policy_sample:
            self.noise.normal_(self._eps_pi)
            self._pi_sampled = True
        native.mlp_forward_multi_sampled(jobs, epis)
        return (a_tanh, logp), c_pi

    # ==========================================================================================
    # target value (reference _get_y 1297-1466 + _v_trace 1244-1295)
    # ==========================================================================================
    def _vtrace_args(self, n_rewards, n_dones, n_last, n_pad, y_out):
        a = native.VtraceArgs()
        a.reward, a.reward_stride = n_rewards.data_ptr(), n_rewards.stride(0)
        a.done, a.last_mask, a.padding_mask = n_dones.data_ptr(), n_last.data_ptr(), n_pad.data_ptr()
        assert n_dones.stride(0) == n_last.stride(0) == n_pad.stride(0)
        a.mask_stride = n_dones.stride(0)
        a.gamma_ratio, a.lambda_ratio = self._gamma_ratio.data_ptr(), self._lambda_ratio.data_ptr()
        a.gamma, a.v_rho, a.v_c = self.gamma, self._v_rho_f, self._v_c_f
        a.use_n_step_is, a.B, a.n = int(self.use_n_step_is), n_rewards.shape[0], self.n_step
        a.y_out = y_out.data_ptr()
        return a

    def _window_sample(self, loc, scale, plain, c_policy, eps_buf, nx_actions, t0_ls=None):
        """Draws into `eps_buf` and samples the policy over the window -> (a_tanh [B, n+1, A], logp [B, n+1], c_pi =
        pi(stored actions) [B, n+1, A] under `use_n_step_is`, else None).  `plain`: one launch; with `t0_ls` (the [B, n+1,
        2A] output `loc | scale` are views of) that launch also draws the policy step's action for t = 0."""
        dsum, A = self.d_action_summed_size, self.c_action_size
        self.noise.normal_(eps_buf)
        if not plain:
            sampled = self._rsample(c_policy, eps_buf)
            c_pi = None
            if self.use_n_step_is:
                c_pi = squash_correction_prob(
                    c_policy, torch.atanh(torch.clamp(nx_actions[..., dsum:], -0.999, 0.999))).contiguous()
            return torch.tanh(sampled), sum_log_prob(squash_correction_log_prob(c_policy, sampled)), c_pi
        f32 = dict(dtype=torch.float32, device=self.device)
        a_tanh, logp = torch.empty(loc.shape, **f32), torch.empty(loc.shape[:-1], **f32)
        c_pi = torch.empty(loc.shape, **f32) if self.use_n_step_is else None
        stored = dict(action=nx_actions, action_offset=dsum, prob_out=c_pi) if self.use_n_step_is else {}
        if t0_ls is not None:
            self.noise.normal_(self._eps_pi)
            native.squash_multi([
                native.squash_job(loc, scale, eps_buf, a_tanh, logp, **stored),
                native.squash_job(t0_ls[:, 0, :A], t0_ls[:, 0, A:], self._eps_pi, self._pi_a, self._pi_logp)])
            self._pi_sampled = True
        else:
            native.squash_sample_fwd(loc, scale, eps_buf, a_tanh, logp, **stored)
        return a_tanh, logp, c_pi

    def _discrete_fused(self, B: int) -> bool:
        """the step's discrete arithmetic runs on the `asac_discrete_*` launches (`fused_discrete_applies`), B rows a batch"""
        return fused_discrete_applies(
            enabled=self._fused_discrete, plain_learner=True, d_action_sizes=self.d_action_sizes,
            c_action_size=self.c_action_size, discrete_dqn_like=self.discrete_dqn_like,
            offline_loss=self.offline_enabled and self.offline_loss, siamese=self.siamese is not None,
            use_prediction=self.use_prediction, data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            ensemble_q_num=self.ensemble_q_num, n_step=self.n_step, batch_size=B)

    def _attach_head_banks(self):
        """`hip_config['fused_discrete_nets']`: every stock critic (online and target) and the stock policy whose `dense` trunk
        is the identity gets the bank of its `d_dense_list` (`fused_heads.attach`: its `forward` then issues one launch per
        pass for the branch stacks); the E online critics' and the E target critics' stacks also form one bank each
        (`_d_q_heads`).  A network with its own `forward`, a trunk, a live dropout, another activation or a width the kernel
        refuses keeps its module code."""
        from . import fused_heads
        from .fused_mlp import _is_identity
        self._q_bank = self._tq_bank = None
        if not (self._fused_discrete_nets and self.d_action_sizes):
            return
        qs, tqs = self.model_q_list, self.model_target_q_list
        stock_q = [type(q).forward is ModelQ.forward and _is_identity(q.dense) for q in qs + tqs]
        attached = [ok and fused_heads.attach(q) for q, ok in zip(qs + tqs, stock_q)]
        pi = self.model_policy
        stock_pi = (all(getattr(type(pi), f) is getattr(ModelPolicy, f) for f in ('forward', 'd_head_raw', 'heads_raw'))
                    and _is_identity(pi.dense))
        pi_attached = stock_pi and fused_heads.attach(pi)
        if all(attached) and not self.c_action_size:
            for name, nets in (('_q_bank', qs), ('_tq_bank', tqs)):
                shape = fused_heads.describe_head_bank([q.d_dense_list for q in nets])
                if shape is not None:
                    setattr(self, name, fused_heads.HeadBank(shape))
        self._logger.info(f'head banks: critics={sum(attached)}/{len(attached)} policy={bool(pi_attached)} '
                          f'ensemble={self._q_bank is not None}')

    def _d_q_heads(self, target: bool, state, obs_list, c_action=None):
        """the discrete head outputs of the E online (or target) critics of a pure-discrete learner on `state` -> a list of
        E [.., D] tensors: views of one [E, .., D] launch output where the ensemble forms a bank, else the loop over the
        critics (`c_action`: what that loop hands a critic for the continuous action it does not have)"""
        bank = self._tq_bank if target else self._q_bank
        if bank is not None:
            return list(bank(state).unbind(0))
        return [q(state, c_action, obs_list)[0] for q in (self.model_target_q_list if target else self.model_q_list)]

    def _hybrid_fused(self, B: int) -> bool:
        """the step's arithmetic on a hybrid action space runs on the `asac_hybrid_*` launches (`fused_hybrid_applies`), B
        rows a batch.  `plain_gaussian`: known without a forward pass for the stock policy's `forward` only (a `Normal`
        on `ModelPolicy.c_bounded`); a policy with its own `forward` keeps the eager code"""
        return fused_hybrid_applies(
            enabled=self._fused_hybrid, plain_learner=type(self)._plain_learner, d_action_sizes=self.d_action_sizes,
            c_action_size=self.c_action_size, discrete_dqn_like=self.discrete_dqn_like,
            offline_loss=self.offline_enabled and self.offline_loss, siamese=self.siamese is not None,
            use_prediction=self.use_prediction, data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            clip_epsilon=self.clip_epsilon, plain_gaussian=type(self.model_policy).forward is ModelPolicy.forward,
            ensemble_q_num=self.ensemble_q_num, n_step=self.n_step, batch_size=B)

    def _dqn_fused(self, B: int, acting: bool = False) -> bool:
        """the step's DQN-like arithmetic runs on the `asac_dqn_*` launches (`fused_dqn_applies`), B rows a batch; `acting`:
        the acting launch, where neither the batch nor the window plays a part"""
        return fused_dqn_applies(
            enabled=self._fused_dqn, plain_learner=True, d_action_sizes=self.d_action_sizes,
            c_action_size=self.c_action_size, discrete_dqn_like=self.discrete_dqn_like,
            offline_loss=self.offline_enabled and self.offline_loss, siamese=self.siamese is not None,
            use_prediction=self.use_prediction, curiosity=self.curiosity is not None, data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            ensemble_q_num=self.ensemble_q_num, n_step=1 if acting else self.n_step, batch_size=1 if acting else B)

    def _rnd_fused(self, rows: int = 1):
        """-> (RndDesc, predictor RndStack, target RndStack, tensors) when random network distillation runs on the
        `asac_rnd_*` launches (`fused_rnd_applies`, with `rnd_n_sample` candidates an entry: a learner whose acting cannot
        take the path does not train on it either), else None.  The stacks are described once: the parameters are views
        of the flat buffers (predictor) or the target's own storage and keep their addresses."""
        if not self.use_rnd or not self._fused_rnd:
            return None
        if self._rnd_stacks is None:
            self._rnd_stacks = False
            from .fused_mlp import describe_rnd_stack, rnd_stack_tensors
            A = self.c_action_size
            if A and not self.d_action_sizes and hasattr(self.model_rnd, 'c_dense'):
                dp = describe_rnd_stack(self.model_rnd.c_dense, self.state_size, A)
                dt = describe_rnd_stack(self.model_target_rnd.c_dense, self.state_size, A)
                if dp is not None and dt is not None and list(dp.residual) == list(dt.residual):
                    pred, targ = rnd_stack_tensors(self.model_rnd.c_dense), rnd_stack_tensors(self.model_target_rnd.c_dense)
                    ok = all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0
                             for x in pred + targ)
                    ok = ok and all(x.grad is not None and x.grad.is_contiguous() and x.grad.data_ptr() % 16 == 0 for x in pred)
                    if ok:
                        self._rnd_stacks = (dp, native.rnd_stack(*pred), native.rnd_stack(*targ), pred + targ)
        stacks = self._rnd_stacks
        ok = fused_rnd_applies(
            enabled=self._fused_rnd, plain_learner=type(self)._plain_learner, d_action_sizes=self.d_action_sizes,
            c_action_size=self.c_action_size, data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            stack_ok=bool(stacks), state_size=self.state_size, n_sample=self.rnd_n_sample, rows=rows)
        return stacks if ok else None

    def _drnd_fused(self, rows: int = 1):
        """-> (residual flags, predictor table, target table, gradient table, tensors) when random network distillation of a
        pure-discrete, policy-based learner runs on the `asac_drnd_*` launches (`fused_rnd_discrete_applies`, with
        `rnd_n_sample` candidates an entry: a learner whose acting cannot take the path does not train on it either), else
        None.  The members are described and the device tables built once: the parameters are views of the flat buffers
        (predictor, and its gradients) or the target's own storage and keep their addresses."""
        if not self.use_rnd or not self._fused_rnd_discrete:
            return None
        if self._drnd_stacks is None:
            self._drnd_stacks = False
            from .fused_mlp import describe_drnd_member, rnd_stack_tensors
            pl, tl = getattr(self.model_rnd, 'd_dense_list', None), getattr(self.model_target_rnd, 'd_dense_list', None)
            D = self.d_action_summed_size
            if (self.d_action_sizes and not self.c_action_size and pl is not None and tl is not None
                    and len(pl) == len(tl) == D <= native.DRND_MAX_MEMBERS):
                flags = {describe_drnd_member(m, self.state_size) for m in list(pl) + list(tl)}
                if len(flags) == 1 and None not in flags:
                    pred, targ = [rnd_stack_tensors(m) for m in pl], [rnd_stack_tensors(m) for m in tl]
                    every = [x for m in pred + targ for x in m]
                    ok = all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0 for x in every)
                    ok = ok and all(x.grad is not None and x.grad.is_contiguous() and x.grad.data_ptr() % 16 == 0
                                    for m in pred for x in m)
                    if ok:
                        self._drnd_stacks = (flags.pop(), native.drnd_table(pred), native.drnd_table(targ),
                                             native.drnd_table([[x.grad for x in m] for m in pred]), every)
        stacks = self._drnd_stacks
        ok = fused_rnd_discrete_applies(
            enabled=self._fused_rnd_discrete, plain_learner=type(self)._plain_learner, d_action_sizes=self.d_action_sizes,
            c_action_size=self.c_action_size, discrete_dqn_like=self.discrete_dqn_like, data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            stack_ok=bool(stacks), state_size=self.state_size, n_sample=self.rnd_n_sample, rows=rows)
        return stacks if ok else None

    @torch.no_grad()
    def _dqn_target_job(self, n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions, n_rewards, n_dones, *,
                        subset_prefix, y_out, q_online, td_out=None):
        """The double-DQN target's inputs (reference `_get_y` 1363-1382 up to the call of `get_dqn_like_d_y`) ->
        `_Return(args, keep)` for `native.dqn_return` / `native.dqn_q_loss_grad`, `args` = (VtraceArgs, DqnJob) and `keep`
        the tensors they point into (alive as long as the record is: hold it until the launch is issued).  It runs the
        target critics over the window and the online critics over its next positions and draws the two subsets (target
        subset first, eval subset second, as the reference draws them).  The policy is not evaluated over the window: this mode never reads it.  `q_online`: the online critics'
        head outputs [B, D] at the step's state (detached)."""
        E = self.ensemble_q_num
        no_c = torch.zeros(0, device=self.device)
        target = self._d_q_heads(True, nx_states, nx_obses_list, no_c)
        sub_next, sub_eval = self._subsets[subset_prefix + '_dnext'], self._subsets[subset_prefix + '_dn']
        self.noise.subset_(sub_next, E)
        next_obs = [o[:, 1:] for o in nx_obses_list]
        eval_next = self._d_q_heads(False, nx_states[:, 1:], next_obs, no_c)
        self.noise.subset_(sub_eval, E)
        args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, y_out)
        args.subset_n, args.subset_next, args.E_sample = sub_eval.data_ptr(), sub_next.data_ptr(), self.ensemble_q_sample
        if td_out is not None:
            args.td_error_out = td_out.data_ptr()
        job = native.dqn_job(self._branches, eval_next, target, action=nx_actions[:, 0], q_online=q_online)
        return _Return((args, job), (eval_next, target, q_online, sub_next, sub_eval))

    def _discrete_logits(self, state, obs_list):
        """the discrete branches' logits [.., D] (the launches normalise them per branch themselves): the stock policy's
        raw head outputs, a plugin policy's distribution logits"""
        if type(self.model_policy).forward is ModelPolicy.forward:
            return self.model_policy.d_head_raw(state)
        return self.model_policy(state, obs_list)[0].logits

    def _discrete_grad_buffers(self, B: int):
        if B not in self._discrete_grads:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._discrete_grads[B] = (torch.zeros(self.ensemble_q_num, B, self.d_action_summed_size, **f32),
                                       torch.zeros(B, self.d_action_summed_size, **f32))
        return self._discrete_grads[B]

    def _hybrid_heads(self, state, obs_list):
        """hybrid learner on the `asac_hybrid_*` launches -> (logits [.., D], loc [.., A], scale [.., A]) with the stock
        policy's trunk evaluated once: the discrete branches' raw head outputs (the launches normalise them per branch
        themselves) and the parameters of the continuous head's Normal; no distribution objects"""
        logits, mean, logstd = self.model_policy.heads_raw(state)
        return (logits, *self.model_policy.c_bounded(mean, logstd))

    def _hybrid_buffers(self, B: int):
        if B not in self._hybrid_bufs:
            f32 = dict(dtype=torch.float32, device=self.device)
            E, D = self.ensemble_q_num, self.d_action_summed_size
            self._hybrid_bufs[B] = dict(
                d_y=torch.zeros(B, **f32), d_y_td=torch.zeros(B, **f32), grad_qd=torch.zeros(E, B, D, **f32),
                grad_cq=torch.zeros(E, B, **f32), grad_logits=torch.zeros(B, D, **f32), grad_logp=torch.zeros(B, **f32))
        return self._hybrid_bufs[B]

    def _stored_action_ratios(self, d_policy, n_mu_probs, nx_actions):
        """discrete branches -> (pi, mu) [B, n]: the stored actions' probability under the policy and under the behaviour
        policy, as products over the branches"""
        dsum = self.d_action_summed_size
        mu = n_mu_probs[..., :dsum] * nx_actions[:, :-1, :dsum]
        mu = torch.where(mu == 0., torch.ones_like(mu), mu).prod(-1).contiguous()
        pi = torch.exp(d_policy.log_prob(nx_actions[..., :dsum]).sum(-1))[:, :-1].contiguous()
        return pi, mu

    def _c_return(self, q_tab, logp, c_pi, n_mu_probs, sub_n, sub_next, n_rewards, n_dones, n_last, n_pad, y_out,
                  q_online=None, td_out=None):
        """The continuous return's arguments -> `_Return(args, keep)`: the filled `VtraceArgs` and the tensors it points
        into that are not the caller's static buffers (alive as long as the record is).  q_tab [E, B, n+1], any strides;
        with `q_online` [E, B] the launch that takes `args` also writes mean_e |q_e - y| into `td_out`."""
        E, Es = self.ensemble_q_num, self.ensemble_q_sample
        args = self._vtrace_args(n_rewards, n_dones, n_last, n_pad, y_out)
        args.q = q_tab.data_ptr()
        args.q_stride_e, args.q_stride_b, args.q_stride_t = q_tab.stride(0), q_tab.stride(1), q_tab.stride(2)
        # (the whole ensemble: the minimum does not depend on the order, no index loads in front of the values)
        args.subset_n, args.subset_next, args.E_sample = (sub_n.data_ptr(), sub_next.data_ptr(), Es) if Es != E else (None, None, Es)
        logp = logp.contiguous()
        args.logp, args.log_alpha = logp.data_ptr(), self.log_c_alpha.data_ptr()
        if self.use_n_step_is:
            args.pi_prob, args.pi_stride_b, args.pi_stride_t = c_pi.data_ptr(), c_pi.stride(0), c_pi.stride(1)
            args.mu_prob, args.mu_stride_b, args.mu_stride_t = \
                n_mu_probs.data_ptr(), n_mu_probs.stride(0), n_mu_probs.stride(1)
            args.mu_offset, args.A = self.d_action_summed_size, self.c_action_size
        if q_online is not None and not self.d_action_sizes:
            q_online = q_online.contiguous()
            args.q_online, args.E_online, args.td_error_out = q_online.data_ptr(), q_online.shape[0], td_out.data_ptr()
        return _Return(args, (q_tab, logp, c_pi, n_mu_probs, sub_n, sub_next, q_online))

    @staticmethod
    def _launch_return(ret, *, sidecars=None, pending_alpha=None, td_update=None) -> bool:
        """Issues the ONE launch that forms the return `ret` (`_c_return`) describes, with `sidecars` as extra workgroups
        and evaluated with the temperature the not-yet-run step `pending_alpha` will write.  `td_update` = (replay buffer,
        ids): where `ret` asks for the TD error that launch is the buffer's priority update too (it then runs the
        temperature step itself) -> True, else False."""
        if td_update is not None and ret.args.td_error_out:
            rb, ids = td_update
            rb.td_update(ret.args, ids, sidecars=sidecars, alpha_step=pending_alpha)
            return True
        native.vtrace_return_min(ret.args, sidecars=sidecars, pending_alpha=pending_alpha)
        return False

    @torch.no_grad()
    def _get_y(self, n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions, n_rewards,
               n_dones, n_mu_probs, *, eps_buf, subset_prefix, y_out, q_online=None, td_out=None, ls=None,
               sample=None, stored_pi=None, policy_sample=False, q_table=None, launch=True, d_q_online=None):
        """-> (d_y [B,1] | None, c_y [B,1] | None);  with `launch=False` -> (d_y, c_y, ret): the continuous return's
        launch is NOT issued, `c_y` is where it will write and `ret` what `_launch_return` (or a launch that forms the
        return itself) needs — None without continuous actions.

        Stock continuous-only networks may hand over work they already did: `ls` = the policy's
        [B, n+1, 2A] (loc | scale) output for `nx_states`; `sample` = (a_tanh [B, n+1, A], logp [B, n+1])
        already drawn from it with `eps_buf`; `stored_pi` = pi(stored actions) [B, n+1, A].  With
        `policy_sample` the launch that samples here also draws the policy step's action for t = 0
        (`self._pi_a`, `self._pi_logp`; same policy parameters, same state).  `q_table` = the target
        ensemble's values [E, B, n+1] on (nx_states, a_tanh) if already computed.

        `nx_actions` is the stored-action window [B, n+1, A] (the reference appends a zero row
        instead, 1329: the extra row's probability is discarded either way).  With `q_online`
        ([E, B], continuous-only action spaces) the TD error mean_e|q_e - y| is produced by the
        same launch into `td_out`; with `d_q_online` (the online critics' discrete head outputs [B, D] each, pure-discrete
        learner on the `asac_discrete_*` launches) likewise; a hybrid learner on the `asac_hybrid_*` launches hands over
        both and gets the summed TD error from its one launch.
        """
        n_actions = nx_actions[:, :-1]
        fused_d = self._discrete_fused(n_rewards.shape[0])
        fused_h = ls is None and sample is None and self._hybrid_fused(n_rewards.shape[0])
        d_logits = None
        if ls is None and sample is None and self._fpi is not None and self.c_action_size and nx_states.dim() == 3:
            # the stock policy over the window and the window's sample as ONE launch (`_return_sample_epilogue`)
            job_pi, ls_out = self._fpi.job(StockMLP._rows_in_place(nx_states, self.state_size), None)
            ls_try = ls_out[0].view(*nx_states.shape[:2], 2 * self.c_action_size)
            pre = self._return_sample_epilogue([job_pi], 0, ls_try, nx_actions, eps_buf, policy_sample)
            if pre is not None:
                ls, (sample, stored_pi) = ls_try, pre
        if ls is not None:
            d_policy = c_policy = None
            loc, scale, plain = ls[..., :self.c_action_size], ls[..., self.c_action_size:], True
        elif fused_d:   # the return's launch forms the branch probabilities from the logits: no distribution objects
            d_policy = c_policy = loc = scale = None
            plain, d_logits = False, self._discrete_logits(nx_states, nx_obses_list)
        elif fused_h:   # ... and the window's sample comes from (loc, scale)
            d_policy = c_policy = None
            (d_logits, loc, scale), plain = self._hybrid_heads(nx_states, nx_obses_list), True
        else:
            d_policy, c_policy, loc, scale, plain = self._policy(nx_states, nx_obses_list)
            ls = self._ls
        self._ls_y = ls    # kept for the policy step (same parameters, state at t = 0 of this window)

        if self.curiosity is not None:   # 1333-1343: augments the sampled reward window in place
            n_states, next_n_states = nx_states[:, :-1], nx_states[:, 1:]
            if self.curiosity == CURIOSITY.FORWARD:
                approx, actual = self.model_forward_dynamic(n_states, n_actions), next_n_states
            else:
                approx, actual = self.model_inverse_dynamic(n_states, next_n_states), n_actions
            if (self._fused_curiosity and approx.is_cuda and approx.dim() == 3 and approx.dtype == torch.float32
                    and actual.stride(-1) == 1 and n_rewards.dim() == 2 and n_rewards.dtype == torch.float32
                    and (n_rewards.stride(1) == 1 or n_rewards.shape[1] == 1) and not torch.is_grad_enabled()):
                native.curiosity_bonus(approx.contiguous(), actual, n_rewards, self.curiosity_strength)   # one launch
            else:
                d = approx - actual
                bonus = torch.sum(d.mul_(d), dim=-1).mul_(0.5)       # 0.5 * sum (approx - actual)^2
                n_rewards.add_(bonus, alpha=self.curiosity_strength)

        logp = c_pi = None
        if self.c_action_size and sample is not None:
            (a_tanh, logp), c_pi = sample, stored_pi
        elif self.c_action_size:
            a_tanh, logp, c_pi = self._window_sample(
                loc, scale, plain, c_policy, eps_buf, nx_actions,
                t0_ls=ls if plain and policy_sample and ls is not None and ls.dim() == 3 else None)
        else:
            a_tanh = torch.zeros(0, device=self.device)

        d_y = c_y = ret = None
        E = self.ensemble_q_num
        nx_qs = None
        if self.d_action_sizes and not self.c_action_size:
            nx_qs = [(h, None) for h in self._d_q_heads(True, nx_states, nx_obses_list, a_tanh)]
        elif self.d_action_sizes:
            nx_qs = [q(nx_states, a_tanh, nx_obses_list) for q in self.model_target_q_list]

        if self.d_action_sizes and self.discrete_dqn_like:   # 1363-1382: double-DQN target, no policy
            sub_next, sub_eval = self._subsets[subset_prefix + '_dnext'], self._subsets[subset_prefix + '_dn']
            self.noise.subset_(sub_next, E)
            target_next = torch.stack([q[0][:, 1:] for q in nx_qs]).index_select(0, sub_next.long())
            next_c = a_tanh[:, 1:] if self.c_action_size else a_tanh
            next_obs = [o[:, 1:] for o in nx_obses_list]
            if self.c_action_size:
                eval_next = torch.stack([q(nx_states[:, 1:], next_c, next_obs)[0] for q in self.model_q_list])
            else:
                eval_next = torch.stack(self._d_q_heads(False, nx_states[:, 1:], next_obs, next_c))
            self.noise.subset_(sub_eval, E)
            d_y = self.get_dqn_like_d_y(n_last_masks, n_padding_masks, n_rewards, n_dones,
                                        eval_next.index_select(0, sub_eval.long()), target_next)
        elif fused_h:   # 1383-1464 on a hybrid space: both heads' V, ratios and scans in ONE launch
            assert launch and q_table is None
            B = n_rewards.shape[0]
            sub_dnext, sub_dn = self._subsets[subset_prefix + '_dnext'], self._subsets[subset_prefix + '_dn']
            self.noise.subset_(sub_dnext, E)
            self.noise.subset_(sub_dn, E)
            sub_cn, sub_cnext = self._subsets[subset_prefix + '_cn'], self._subsets[subset_prefix + '_cnext']
            self.noise.subset_(sub_cn, E)
            self.noise.subset_(sub_cnext, E)
            d_out = self._hybrid_buffers(B)['d_y_td' if subset_prefix == 'td' else 'd_y']
            d_args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, d_out)
            d_args.subset_n, d_args.subset_next, d_args.E_sample = sub_dn.data_ptr(), sub_dnext.data_ptr(), self.ensemble_q_sample
            d_args.log_alpha = self.log_d_alpha.data_ptr()
            if self.use_n_step_is:
                d_args.mu_prob, d_args.mu_stride_b, d_args.mu_stride_t = \
                    n_mu_probs.data_ptr(), n_mu_probs.stride(0), n_mu_probs.stride(1)
            q_tab = torch.stack([q[1] for q in nx_qs]).squeeze(-1)            # [E, B, n+1]
            ret = self._c_return(q_tab, logp, c_pi, n_mu_probs, sub_cn, sub_cnext, n_rewards, n_dones, n_last_masks,
                                 n_padding_masks, y_out)
            ret.args.A = self.c_action_size
            with_td = d_q_online is not None    # mean_e (|(1/K) sum_j a_j q_e - d_y| + |c_q_e - c_y|) from the same launch
            native.hybrid_return(d_args, ret.args, self._branches, [q[0] for q in nx_qs], d_logits, action=nx_actions,
                                 q_online=d_q_online, c_q_online=q_online if with_td else None,
                                 td_out=td_out if with_td else None)
            return d_out.unsqueeze(-1), y_out.unsqueeze(-1)
        elif fused_d:   # 1383-1421, policy-based branch: subset means, branch softmax, V, ratios and the scan in ONE launch
            sub_next, sub_n = self._subsets[subset_prefix + '_dnext'], self._subsets[subset_prefix + '_dn']
            self.noise.subset_(sub_next, E)
            self.noise.subset_(sub_n, E)
            args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, y_out)
            args.subset_n, args.subset_next, args.E_sample = sub_n.data_ptr(), sub_next.data_ptr(), self.ensemble_q_sample
            args.log_alpha = self.log_d_alpha.data_ptr()
            if self.use_n_step_is:
                args.mu_prob, args.mu_stride_b, args.mu_stride_t = \
                    n_mu_probs.data_ptr(), n_mu_probs.stride(0), n_mu_probs.stride(1)
            if d_q_online is not None:    # the TD error mean_e |(1/K) sum_j a_j q_e - y| from the same launch
                args.td_error_out = td_out.data_ptr()
            native.discrete_return(args, self._branches, [q[0] for q in nx_qs], d_logits, action=nx_actions,
                                   q_online=d_q_online)
            d_y = y_out.unsqueeze(-1)
        elif self.d_action_sizes:   # 1383-1421, policy-based branch, eager ops + the scan kernel
            sub_next, sub_n = self._subsets[subset_prefix + '_dnext'], self._subsets[subset_prefix + '_dn']
            self.noise.subset_(sub_next, E)
            self.noise.subset_(sub_n, E)
            stacked = torch.stack([q[0] for q in nx_qs])                      # [E, B, n+1, D]
            mean_next = stacked[:, :, 1:].index_select(0, sub_next.long()).mean(0)
            mean_n = stacked[:, :, :-1].index_select(0, sub_n.long()).mean(0)
            probs = d_policy.probs
            n_p, next_p = probs[:, :-1], probs[:, 1:]
            d_alpha = torch.exp(self.log_d_alpha)
            v_n = torch.sum(n_p * (mean_n - d_alpha * torch.log(n_p.clamp(min=1e-8))), -1) / self.d_action_branch_size
            v_next = torch.sum(next_p * (mean_next - d_alpha * torch.log(next_p.clamp(min=1e-8))), -1) \
                / self.d_action_branch_size
            pi, mu = self._stored_action_ratios(d_policy, n_mu_probs, nx_actions) if self.use_n_step_is else (None, None)
            d_y = torch.empty(n_rewards.shape[0], dtype=torch.float32, device=self.device)
            args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, d_y)
            native.vtrace_return_direct(args, v_n.contiguous(), v_next.contiguous(), pi, mu)
            d_y = d_y.unsqueeze(-1)

        if self.c_action_size:    # 1423-1464, fused
            sub_n, sub_next = self._subsets[subset_prefix + '_cn'], self._subsets[subset_prefix + '_cnext']
            self.noise.subset_(sub_n, E)
            self.noise.subset_(sub_next, E)
            if q_table is not None:
                q_tab = q_table
            elif nx_qs is not None:
                q_tab = torch.stack([q[1] for q in nx_qs]).squeeze(-1)        # [E, B, n+1]
            else:
                q_tab = self._c_q_values(True, nx_states, a_tanh, nx_obses_list)
            ret = self._c_return(q_tab, logp, c_pi, n_mu_probs, sub_n, sub_next, n_rewards, n_dones, n_last_masks,
                                 n_padding_masks, y_out, q_online, td_out)
            if launch:
                self._launch_return(ret)
            c_y = y_out.unsqueeze(-1)
        return (d_y, c_y) if launch else (d_y, c_y, ret)

    # ==========================================================================================
    # losses / updates (reference _train_rep_q 1468-1605, _train_policy 1841-1911, _train_alpha 1913-1949)
    # ==========================================================================================
    def _stock_q_targets(self, job_tq, job_pi, ls, window, policy_sample):
        """One launch: the target Q of the stored pair (`job_tq`, for the clipped loss) beside the policy over the window
        (`job_pi`, `ls` its output) — whose lanes also draw the window's sample (`_return_sample_epilogue`; otherwise an
        elementwise launch in `_get_y`).  Then the return target over `window` (`_get_y`'s positional arguments), its
        launch not issued -> (c_y, ret)."""
        nx_states, nx_actions = window[3], window[4]
        ls = ls[0].view(*nx_states.shape[:2], 2 * self.c_action_size)
        pre = self._return_sample_epilogue([job_tq, job_pi], 1, ls, nx_actions, self._eps_y, policy_sample)
        if pre is None:
            native.mlp_forward_multi([job_tq, job_pi])
        sample, stored_pi = pre or (None, None)
        _, c_y, ret = self._get_y(*window, eps_buf=self._eps_y, subset_prefix='y', y_out=self._y_buf, ls=ls,
                                  sample=sample, stored_pi=stored_pi, policy_sample=policy_sample and pre is None,
                                  launch=False)
        return c_y, ret

    def _rider_plan(self, x_pi, ret):
        """the save buffer when the Q-loss backward launch may carry the policy's forward on the rows `x_pi` and the policy
        step will be the one-launch form that loads it, else None; decided once per (rows, return shape), not per call"""
        key = (x_pi.data_ptr(), x_pi.stride(0), x_pi.shape[0], ret.args.n)
        cached = self._rider_plan_cache
        if cached is not None and cached[0] == key:
            return cached[1]
        B, fq, fpi = x_pi.shape[0], self._fq, self._fpi
        save = None
        if self._fused_policy_step and self.ensemble_q_sample == 2 and fpi.policy_step_fused_ok(fq, B):
            save = fpi.forward_save_buffer(B)
            if not (fq.backward_qloss_return_rider_ok(B, ret.args, fpi, x_pi, save) and
                    native.policy_step_fused_loaded_ok(fq.desc, fq.params, fq.member_stride, fpi.desc, fpi.params,
                                                       fpi.member_stride, B, save)):
                save = None
        self._rider_plan_cache = (key, save)
        return save

    @staticmethod
    def _critic_plan_key(x0, a0, T):
        return (x0.data_ptr(), x0.stride(0), a0.data_ptr(), a0.stride(0), x0.shape[0], T)

    def _critic_rider_plan(self, key, x0, ret):
        """decides, once per static set (`key`: the stored pair's rows and the window), whether the step's first network
        launch carries the online critics' forward for a Q-loss backward that loads it; allocates the save buffer — in the
        eager warm-up: never while a capture is running.  The first step of a set therefore issues today's launches; the
        forward launch still asks its own predicate each time (its grid depends on the sidecars it carries)."""
        if key in self._critic_plan_cache or torch.cuda.is_current_stream_capturing():
            return
        B, fq = x0.shape[0], self._fq
        save = None
        if self._critic_forward_rider and self._fused_q_return and self._dist is None and x0.dim() == 2 \
                and fq.backward_qloss_return_ok(B, ret.args):
            save = fq.critic_save_buffer(B)
            if not fq.backward_qloss_return_loaded_ok(B, ret.args, save):
                save = None
        self._critic_plan_cache[key] = save

    def _stock_q_backward(self, x0, a0, ret, c_y, priority_is, fold, fused_return, state_grads=False, rider_rows=None,
                          critic_saved=None):
        """[online critics forward, clipped double-Q loss, backward] in one launch (the backward recomputes the forward
        on chip anyway).  With `fused_return` its own workgroups form the return target `ret` where that form applies
        (short windows); otherwise the return's launch goes first.  `fold`: the tile reduction of the parameter
        gradients is folded into the Adam launch, issued here.  -> d loss / d x0 [E, B, S] with `state_grads`.
        `rider_rows`: the policy step's state rows [B, S] when its action is already drawn — the launch then runs the
        policy's forward on them on further workgroups (`_rider_plan`) and `_pi_saved` hands it to the policy step.
        `critic_saved`: the online critics' forward on (x0, a0) as this step's first network launch saved it — loaded
        instead of recomputed where the loaded form applies (no `state_grads`)."""
        w = priority_is.reshape(-1).contiguous() if priority_is is not None else None
        t_q = self._tq_buf.view(self.ensemble_q_num, -1)
        self._pi_saved = None
        if fused_return and self._fq.backward_qloss_return_ok(x0.shape[-2], ret.args):
            save = self._rider_plan(rider_rows, ret) if rider_rows is not None else None
            # (the critics' forward is loaded where the first network launch saved it and the loaded form applies)
            if critic_saved is not None and (state_grads or not self._fq.backward_qloss_return_loaded_ok(
                    x0.shape[-2], ret.args, critic_saved, *((self._fpi, rider_rows, save) if save is not None else ()))):
                critic_saved = None
            if save is not None:
                g0 = self._fq.backward_qloss_return_rider(x0, a0, t_q, ret.args, w, self.clip_epsilon, self._loss_q_e,
                                                          self._fpi, rider_rows, save, defer=fold, state_grads=state_grads,
                                                          critic_saved=critic_saved)
                self._pi_saved = (save, rider_rows.data_ptr(), rider_rows.stride(0), rider_rows.shape[0])
            else:
                g0 = self._fq.backward_qloss_return(x0, a0, t_q, ret.args, w, self.clip_epsilon, self._loss_q_e,
                                                    defer=fold, state_grads=state_grads, critic_saved=critic_saved)
        else:
            self._launch_return(ret)
            g0 = self._fq.backward_qloss(x0, a0, t_q, c_y.reshape(-1), w, self.clip_epsilon, self._loss_q_e,
                                         defer=fold, state_grads=state_grads)
        if fold:
            self._fq.adam_partials(self.optimizer_q_list[0], loss_out=self._loss_q_e)
        return g0

    @torch.no_grad()
    def _train_rep_q_stock(self, n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions, n_rewards,
                           n_dones, n_mu_probs, priority_is, policy_sample):
        """Q step (reference 1468-1605) for stock networks under a parameter-free representation as an
        explicit kernel chain: target Q of the stored (s0, a0) pair -> return target -> [online Q, clipped
        double-Q loss, backward] in one launch -> [tile reduction + Adam] in one launch."""
        E, B = self.ensemble_q_num, nx_states.shape[0]
        x0 = StockMLP._rows(nx_states[:, 0], self.state_size)
        a0 = StockMLP._rows(nx_actions[:, 0], self.c_action_size)
        xs = StockMLP._rows(nx_states, self.state_size)
        job_tq, _ = self._ftq.job(x0, a0, out=self._tq_buf)
        job_pi, ls = self._fpi.job(xs, None)
        T, A = nx_states.shape[1], self.c_action_size
        window = (n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions, n_rewards, n_dones,
                  n_mu_probs if self.use_n_step_is else None)
        fused = None
        if self._fused_forward_chain and self.curiosity is None:
            # policy over the window -> target sample (+ pi(stored actions), + the policy step's sample at t = 0) ->
            # target critics on the sampled actions, with the target Q of the stored pair riding along: ONE launch
            # (bit-identical to the three it replaces)
            f32 = dict(dtype=torch.float32, device=self.device)
            a_y, logp_y = torch.empty((B, T, A), **f32), torch.empty((B, T), **f32)
            c_pi = torch.empty((B, T, A), **f32) if self.use_n_step_is else None
            job_q, q_tab = self._ftq.job(xs, a_y.view(-1, A))
            fused = native.pi_q_job(job_pi, job_q, self._eps_y, a_y, logp_y, T,
                                    action=nx_actions if self.use_n_step_is else None,
                                    action_offset=self.d_action_summed_size, prob_out=c_pi,
                                    eps2=self._eps_pi if policy_sample else None, t2=0,
                                    a2_out=self._pi_a, logp2_out=self._pi_logp)
            if not native.policy_sample_q_forward_ok(fused):
                fused = None
        riders = None
        if fused is not None and self._head_gather is not None:
            # the step's gather is still pending: this launch reads its rows (states, stored actions, the stored pair) from
            # the replay ring and carries the gather for the launches behind it
            ring = self._head_ring_job(fused, job_tq, self._head_gather, nx_states, nx_actions)
            if ring is not None:
                fused, riders = ring, [self._head_gather['sidecar_w' if self._head_gather_w else 'sidecar']]
                self._head_gather = None
        self._join_head_gather()
        critic_saved, critic_key = None, None
        if fused is not None:
            self.noise.normal_(self._eps_y)
            if policy_sample:
                self.noise.normal_(self._eps_pi)
                self._pi_sampled = True
            sidecars = riders if riders is not None else self._take_la_gather()
            # the online critics' forward on the stored pair rides along where the plan of this static set says so and the
            # launch has the CUs for it; the Q-loss backward below then loads it (same launches, bit-identical)
            critic_key = self._critic_plan_key(x0, a0, T)
            plan = self._critic_plan_cache.get(critic_key) if self._critic_forward_rider else None
            if plan is not None:
                job_online = self._fq._pass(x0, a0)
                if native.policy_sample_q_forward_saving_ok(fused, [job_tq], sidecars, job_online, plan):
                    critic_saved = plan
            if critic_saved is not None:
                native.policy_sample_q_forward_saving(fused, [job_tq], sidecars, job_online, critic_saved)
            else:
                native.policy_sample_q_forward(fused, [job_tq], sidecars=sidecars)
            _, c_y, ret = self._get_y(*window, eps_buf=self._eps_y, subset_prefix='y', y_out=self._y_buf,
                                      ls=ls[0].view(B, T, 2 * A), sample=(a_y, logp_y), stored_pi=c_pi,
                                      q_table=q_tab.view(E, B, T), launch=False)
        else:
            c_y, ret = self._stock_q_targets(job_tq, job_pi, ls, window, policy_sample)
        # on a single GPU the tile reduction of the parameter gradients is folded into the Adam launch
        opt = self.optimizer_q_list[0]
        fold = self._dist is None and opt.start == self._fq._start and self._params.span('rep')[0] == self._params.span('rep')[1]
        # (behind the one-launch forward the backward may form the return itself; behind the chain form it never did)
        # (... and, with the policy step's action drawn by that forward, carry the policy's forward for the policy step)
        rider_rows = x0 if (self._policy_forward_rider and fused is not None and policy_sample and x0.dim() == 2) else None
        if critic_key is not None and self._critic_forward_rider:
            self._critic_rider_plan(critic_key, x0, ret)
        self._stock_q_backward(x0, a0, ret, c_y, priority_is, fold, fused_return=fused is not None and self._fused_q_return,
                               rider_rows=rider_rows, critic_saved=critic_saved)
        if not fold:
            self._finish_rep_q(None, None)

    def _head_ring_job(self, fused, job_tq, head, nx_states, nx_actions):
        """`fused` (the one-launch forward chain over `nx_states` / `nx_actions`, views of the static batch from window row
        b on) and `job_tq` (the stored pair at row b, riding along) with ring-addressed rows, or None where the views are not
        the gathered observation / action buffers or the launch refuses the pair of jobs"""
        rb, b = self.replay_buffer, self.burn_in_step
        obs, act = rb._batch[f'obs_{self.obs_names[0]}'], rb._batch['action']
        if b != rb.prev_n or nx_states.shape[1] + b != rb.window:
            return None
        for view, whole in ((nx_states, obs), (nx_actions, act)):
            at = whole[:, b:]
            if view.data_ptr() != at.data_ptr() or view.stride() != at.stride() or view.shape != at.shape:
                return None
        job = native.pi_q_ring_rows(fused, rb._ids, head['index_ring'], rb.capacity, rb.prev_n, rb.window, b, head['x0'],
                                    head['action'], x_j0=b, x_action_offset=self.d_action_summed_size)
        return job if native.policy_sample_q_forward_ok(job, [job_tq]) else None

    def _train_rep_q(self, n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions, n_rewards,
                     n_dones, n_mu_probs, priority_is, aux=None, policy_sample=False, state_base=None):
        """`policy_sample`: see `_get_y`.  `state_base` = (window states [B, L, S], t) with
        `nx_states[:, 0] == window[:, t]`.  `aux` (only with siamese / prediction heads): dict(n_indexes, n_pre_actions,
        n_pre_seq_hidden_states, nx_target_states) for the auxiliary losses of reference 1577-1600."""
        if (self._stock_c_only() and aux is None and self.clip_epsilon > 0 and not nx_states.requires_grad
                and self.optimizer_rep is None):
            return self._train_rep_q_stock(n_last_masks, n_padding_masks, nx_obses_list, nx_states, nx_actions,
                                           n_rewards, n_dones, n_mu_probs, priority_is, policy_sample)
        self._join_head_gather()
        dsum = self.d_action_summed_size
        obs_list = [o[:, 0] for o in nx_obses_list]
        state, action = nx_states[:, 0], nx_actions[:, 0]
        if state_base is not None and not nx_states.requires_grad:
            state = state_base[0][:, state_base[1]]     # (`_step_rep_and_q`: the differentiable pass covered this position only)
        d_action, c_action = action[..., :dsum], action[..., dsum:]

        if (self._fused_q_state_grads and self._fq is not None and self._ftq is not None and self._fpi is not None
                and not self.d_action_sizes
                and self.c_action_size and self.clip_epsilon > 0 and aux is None and state_base is not None
                and state_base[0].dim() == 3 and state.requires_grad):
            # stock critics behind a trainable representation: target Q of the stored pair -> return target -> ONE
            # launch for [critics forward, clipped double-Q loss, backward] that also returns d loss / d state (the
            # separate critic forward and loss launches of the autograd form disappear); the representation's backward
            # continues from that gradient
            base, t = state_base
            with torch.no_grad():
                x0 = StockMLP._rows(base.detach()[:, t], self.state_size)
                a0 = StockMLP._rows(c_action, self.c_action_size)
                states_y = nx_states.detach()
                job_tq, _ = self._ftq.job(x0, a0, out=self._tq_buf)
                job_pi, ls_y = self._fpi.job(StockMLP._rows_in_place(states_y, self.state_size), None)
                c_y, ret = self._stock_q_targets(
                    job_tq, job_pi, ls_y, (n_last_masks, n_padding_masks, nx_obses_list, states_y, nx_actions, n_rewards,
                                           n_dones, n_mu_probs if self.use_n_step_is else None), policy_sample)
                # one GPU: the critics' tile reduction is folded into their Adam launch (as without a trainable
                # representation), which then no longer waits for the representation's backward
                fold = self._dist is None and self._fold_rep_q_adam and self._rep_q_adam_alike()
                g0 = self._stock_q_backward(x0, a0, ret, c_y, priority_is, fold, fused_return=self._fused_q_return,
                                            state_grads=True)
                # d loss / d (window states): zero except at position t — a buffer that stays zero elsewhere, so only the
                # slice is written each step (no memset launch)
                g_base = self._g_state_base
                if g_base is None or g_base.shape != base.shape:
                    g_base = self._g_state_base = torch.zeros_like(base)
                at_position = self._gru_backward_at and fused_gru.is_fused_top(base)
                from_head = not at_position and self._head_sums_members and fused_linear.is_fused_head_output(base)
                if not (at_position or from_head):
                    torch.sum(g0, dim=0, out=g_base[:, t])
            rep_stepped = False
            # (the backward launches' second launches — per-workgroup partials summed into the flat gradient — run as one
            # launch when the walk is done, in front of the optimizer step: param_grads.learner_backward)
            with learner_backward():
                if at_position:
                    # the window IS a fused GRU's output: its backward sums the members' gradients itself and starts at
                    # position t (the steps behind it only feed detached targets) — no member-sum launch in between;
                    # where that GRU is all the representation has, the launch finishing its gradients steps it too
                    rep_stepped = fused_gru.backward_from_position(base, g0, t, g_base,
                                                                   adam=self._rep_adam_epilogue() if fold else None)
                elif from_head:
                    # the window is a fused Linear + Tanh head's output: its backward launch sums the members
                    fused_linear.backward_from_members(base, g0, t, g_base)
                else:
                    torch.autograd.backward([base], [g_base])
            if fold:
                if not rep_stepped:
                    self.optimizer_q_list[0].step(*self._params.span('rep'))
                return
            return self._finish_rep_q(None, None)
        q_list = None
        if self.d_action_sizes and not self.c_action_size:
            q_list, c_q = [(h, None) for h in self._d_q_heads(False, state, obs_list, c_action)], None
        elif self.d_action_sizes:
            q_list = [q(state, c_action, obs_list) for q in self.model_q_list]
            c_q = torch.stack([q[1] for q in q_list]).squeeze(-1)
        else:
            c_q = self._c_q_values(False, state, c_action, obs_list, select=state_base)   # [E, B]
        if self.d_action_sizes and aux is None and self._dqn_fused(state.shape[0]):
            # DQN-like: the loss launch forms the double-DQN target itself (row-local, y stays in registers), then loss
            # values and d(sum_e l_e) / d(head outputs); back-propagation starts at the heads
            heads = [q[0] for q in q_list]
            grad_q, _ = self._discrete_grad_buffers(state.shape[0])
            ret = self._dqn_target_job(n_last_masks, n_padding_masks, nx_obses_list, nx_states.detach(), nx_actions,
                                       n_rewards, n_dones, subset_prefix='y', y_out=self._y_buf,
                                       q_online=[h.detach() for h in heads])
            native.dqn_q_loss_grad(*ret.args, priority_is, self._loss_q_e, grad_q)
            del ret
            with learner_backward():
                torch.autograd.backward(heads, list(grad_q.unbind(0)))
            return self._finish_rep_q(None, None)
        d_y, c_y = self._get_y(n_last_masks, n_padding_masks, nx_obses_list, nx_states.detach(), nx_actions,
                               n_rewards, n_dones, n_mu_probs if self.use_n_step_is else None,
                               eps_buf=self._eps_y, subset_prefix='y', y_out=self._y_buf,
                               policy_sample=policy_sample)

        losses = None
        if self.d_action_sizes and aux is None and self._discrete_fused(state.shape[0]):
            # loss values and d(sum_e l_e) / d(head outputs) from one launch; back-propagation starts at the heads
            heads = [q[0] for q in q_list]
            grad_q, _ = self._discrete_grad_buffers(state.shape[0])
            native.discrete_q_loss_grad(self._branches, [h.detach() for h in heads], d_action, d_y, priority_is,
                                        self._loss_q_e, grad_q)
            with learner_backward():
                torch.autograd.backward(heads, list(grad_q.unbind(0)))
            return self._finish_rep_q(None, None)
        if self.d_action_sizes and aux is None and self._hybrid_fused(state.shape[0]):
            # hybrid: both heads' loss terms and d(sum_e l_e) / d(discrete head outputs, continuous values) from one launch;
            # back-propagation starts at the heads and the stacked continuous values
            heads = [q[0] for q in q_list]
            with torch.no_grad():
                t_q = self._c_q_values(True, state.detach(), c_action, obs_list)
            buf = self._hybrid_buffers(state.shape[0])
            native.hybrid_q_loss_grad(self._branches, [h.detach() for h in heads], d_action, c_q.detach().contiguous(),
                                      t_q.contiguous(), d_y, c_y, priority_is, self.clip_epsilon, self._loss_q_e,
                                      buf['grad_qd'], buf['grad_cq'])
            with learner_backward():
                torch.autograd.backward(heads + [c_q], list(buf['grad_qd'].unbind(0)) + [buf['grad_cq']])
            return self._finish_rep_q(None, None)
        if self.d_action_sizes:
            qs = torch.stack([torch.sum(d_action * q[0], dim=-1, keepdim=True) / self.d_action_branch_size
                              for q in q_list])                                   # [E, B, 1]
            losses = functional.mse_loss(qs, d_y.expand_as(qs), reduction='none')
        if self.c_action_size:
            if self.clip_epsilon > 0:
                with torch.no_grad():
                    t_q = self._c_q_values(True, state.detach(), c_action, obs_list)
                if losses is None and (aux is None or self._fused_q_loss_with_aux):
                    # loss value and d(sum_e l_e)/dq from one launch; back-propagation starts at q (with auxiliary heads
                    # too: they only need the graph kept for the prediction models' second pass and the main gradients
                    # in place before they gate theirs)
                    w = priority_is.reshape(-1).contiguous() if priority_is is not None else None
                    native.q_loss_fwd_bwd(c_q.detach().contiguous(), t_q.contiguous(), c_y.reshape(-1), w,
                                          self.clip_epsilon, self._loss_q_e, self._grad_q)
                    with learner_backward():
                        torch.autograd.backward([c_q], [self._grad_q],
                                                retain_graph=aux is not None and self.use_prediction)
                    if aux is None:
                        return self._finish_rep_q(None, None)
                    return self._finish_rep_q(None, None, aux,
                                              dict(n_padding_masks=n_padding_masks, nx_obses_list=nx_obses_list,
                                                   nx_states=nx_states, nx_actions=nx_actions, n_rewards=n_rewards))
                clipped = t_q + torch.clamp(c_q - t_q, -self.clip_epsilon, self.clip_epsilon)
                yv = c_y.reshape(1, -1)
                c_loss = torch.maximum((clipped - yv) ** 2, (c_q - yv) ** 2).unsqueeze(-1)
            else:   # 1556: `+=` of (self + mse) doubles the running loss
                c_loss = functional.mse_loss(c_q, c_y.reshape(1, -1).expand_as(c_q), reduction='none').unsqueeze(-1)
                losses = losses * 2 if losses is not None else None
            losses = c_loss if losses is None else losses + c_loss
        if priority_is is not None:
            losses = losses * priority_is.unsqueeze(0)
        loss_q_list = losses.mean(dim=(1, 2))
        return self._finish_rep_q(loss_q_list.sum(), loss_q_list[0], aux,
                                  dict(n_padding_masks=n_padding_masks, nx_obses_list=nx_obses_list,
                                       nx_states=nx_states, nx_actions=nx_actions, n_rewards=n_rewards))

    def _rep_q_adam_alike(self) -> bool:
        """the representation's and the critics' optimizers have the same hyper-parameters: only then may ONE Adam launch
        step both spans (`fold_rep_q_adam`); a schedule or a user edit that moves one of them un-folds the step"""
        a, b = self.optimizer_rep, self.optimizer_q_list[0]
        return a is None or (a.lr, tuple(a.betas), a.eps) == (b.lr, tuple(b.betas), b.eps)

    def _rep_adam_epilogue(self):
        """-> `native.adam_epilogue` for the representation's parameters when they are exactly one fused GRU layer's
        cell weights (then the launch that finishes their gradients can step them), else None"""
        hp = (self.optimizer_rep.lr, *self.optimizer_rep.betas, self.optimizer_rep.eps) if self.optimizer_rep is not None else None
        if self._rep_epilogue is False or self._rep_epilogue_hp != hp:      # (a changed learning rate rebuilds it)
            self._rep_epilogue, self._rep_epilogue_hp = None, hp
            from .nn_models.layers.seq_layers import GRU
            grus = [m for m in self.model_rep.modules() if isinstance(m, GRU)]
            opt, (s, e) = self.optimizer_q_list[0], self._params.span('rep')
            if (len(grus) == 1 and grus[0]._fusable and self.optimizer_rep is not None and e > s
                    and {id(p) for p in grus[0].parameters()} == {id(p) for p in self.model_rep.parameters()}):
                g = self._params
                self._rep_epilogue = native.adam_epilogue(g.flat[s:e], g.grad[s:e], opt.exp_avg[s:e], opt.exp_avg_sq[s:e],
                                                          self.optimizer_rep.lr, *self.optimizer_rep.betas,
                                                          self.optimizer_rep.eps, opt.steps_done)
        return self._rep_epilogue

    def _finish_rep_q(self, total_loss, loss_q0, aux=None, ctx=None):
        if total_loss is not None:
            # the prediction heads differentiate the representation graph again (sac_aux._train_rpm)
            # the main loss accumulates into every parameter it reaches (representation + Q ensemble): the fused
            # layers add their parameter gradients in place
            with learner_backward():
                total_loss.backward(retain_graph=aux is not None and self.use_prediction)
            self._stats['loss_q'].copy_(loss_q0.detach())
        start, stop = self._params.span('rep', f'q_{self.ensemble_q_num - 1}')
        if aux is None:
            if self._dist is not None:
                self._dist.all_reduce_grads(self._params.grad, start, stop)
            # Q optimizers then the representation optimizer (1589-1603): adjacent segments, one launch
            self.optimizer_q_list[0].step(start, stop)
            return
        # with auxiliary heads the reference order matters: siamese -> Q step -> prediction -> rep step
        grads_rep_main = [p.grad.detach() for p in self.model_rep.parameters()]
        grads_q_main = [[p.grad.detach() for p in q.parameters()] for q in self.model_q_list]
        if self.siamese is not None:
            n_obs = [o[:, :-1] for o in ctx['nx_obses_list']]
            self._train_siamese_representation_learning(grads_rep_main, grads_q_main, aux['n_indexes'],
                                                        ctx['n_padding_masks'], n_obs, aux['n_pre_actions'],
                                                        aux['n_pre_seq_hidden_states'])
        # data parallel: every segment is averaged over the ranks AFTER the auxiliary heads have added their (gated)
        # gradients to it and right before its optimizer steps, so the replicas stay identical
        q_start = self._params.span('q_0')[0]
        if self._dist is not None:
            self._dist.all_reduce_grads(self._params.grad, q_start, stop)
        self.optimizer_q_list[0].step(q_start, stop)
        if self.use_prediction:
            self._train_rpm(grads_rep_main, ctx['nx_obses_list'], ctx['nx_states'], aux['nx_target_states'],
                            ctx['nx_actions'][:, :-1], ctx['n_rewards'])
        if self.optimizer_rep is not None:
            if self._dist is not None:
                self._dist.all_reduce_grads(self._params.grad, *self._params.span('rep'))
            self.optimizer_rep.step()

    def _stock_c_only(self) -> bool:
        """Stock Q ensemble and stock policy on a continuous-only action space: the whole policy / alpha
        / write-back chain runs on libasac_hip kernels without autograd."""
        return (self._fpi is not None and self._fq is not None and bool(self.c_action_size)
                and not self.d_action_sizes and (not (self.offline_enabled and self.offline_loss) or self._offline_fused()))

    def _offline_fused(self) -> bool:
        """the offline loss' term rides in the stock policy step's launches (`fused_offline_applies`)"""
        return fused_offline_applies(
            enabled=self._fused_offline, plain_learner=type(self)._plain_learner,
            offline_loss=self.offline_enabled and self.offline_loss, c_action_size=self.c_action_size,
            d_action_sizes=self.d_action_sizes, stock_networks=self._fq is not None and self._fpi is not None,
            data_parallel=self._dist is not None,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda)

    def _offline_plain(self) -> bool:
        """the offline loss' term joins the plain-Gaussian autograd path of `_train_policy` (plugin critics) through
        `asac_policy_offline_term`; an `OptionBase`, a data-parallel context or the switch off keep the eager tail"""
        return bool(self._fused_offline and type(self)._plain_learner and self._dist is None
                    and self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda)

    @torch.no_grad()
    def _train_policy_stock(self, state, ls=None, offline=None):
        """Policy step (reference 1841-1911) for the stock networks as an explicit kernel chain:
        [policy forward] -> rsample/tanh/log-prob -> Q ensemble forward -> objective + its gradients
        -> Q backward (input gradients only) -> sampling backward (sums the members' action gradients)
        -> policy backward -> Adam.  `ls` = the policy's [B, 2A] (loc | scale) output for `state` if
        the caller already has it (same parameters, same input).  `offline`: the stored actions [B, A] (a strided view of
        the window) when the offline loss is on — its term is formed inside the sampling backward of either route."""
        A, E = self.c_action_size, self.ensemble_q_num
        x = StockMLP._rows(state, self.state_size)
        B = x.shape[0]
        fusable = (self._fused_policy_step and self.ensemble_q_sample == 2 and self._fpi.policy_step_fused_ok(self._fq, B))
        sample_out = None
        saved, self._pi_saved, given = self._pi_saved, None, False
        if ls is None and not self._pi_sampled and fusable:
            # nothing of the policy's forward is at hand (trainable representation: the state is new): the one-launch
            # policy step samples the action itself
            f32 = dict(dtype=torch.float32, device=self.device)
            self.noise.normal_(self._eps_pi)
            sample_out = (torch.empty((B, A), **f32), torch.empty(B, **f32), torch.empty((B, 2 * A), **f32))
            a_tanh, logp, scale = sample_out[0], sample_out[1], sample_out[2][:, A:]
        else:
            if ls is None:
                ls = self._fpi._launch_forward(x, None)[0]
            loc, scale = ls[..., :A], ls[..., A:]
            if self._pi_sampled:        # drawn by the target computation's launch from the same `ls`
                a_tanh, logp, self._pi_sampled, given = self._pi_a, self._pi_logp, False, True
            else:
                self.noise.normal_(self._eps_pi)
                a_tanh = torch.empty((B, A), dtype=torch.float32, device=self.device)
                logp = torch.empty(B, dtype=torch.float32, device=self.device)
                native.squash_sample_fwd(loc, scale, self._eps_pi, a_tanh, logp)
        sub = self._subsets['pi_c']
        self.noise.subset_(sub, E)
        # (with the offline loss the logged objective also needs the (loc | scale) rows, the noise and the stored actions)
        self._pi_stats_src = (logp, scale) if offline is None else (
            logp, scale, sample_out[2] if sample_out is not None else ls, self._eps_pi, offline)
        opt = self.optimizer_policy
        fold = self._dist is None and (opt.start, opt.stop) == (self._fpi._start, self._fpi._start + self._fpi.member_stride)
        if (fusable and given and saved is not None and a_tanh.is_contiguous()
                and saved[1:] == (x.data_ptr(), x.stride(0), B)):
            # ... with the policy's forward on exactly these rows saved by the Q-loss backward launch's rider: loaded, not
            # run again (same launch count, bit-identical)
            self._fpi.policy_step_fused_loaded(self._fq, x, a_tanh, self._eps_pi, self.log_c_alpha, saved[0],
                                               q_out=self._pi_q, defer=fold, subset=sub if E != 2 else None,
                                               offline=offline)
        elif fusable and a_tanh.is_contiguous():
            # two critics sampled (of two or more): critics forward, objective gradient, critics backward to the action,
            # sampling backward and policy backward in ONE launch (bit-identical to the chain below)
            self._fpi.policy_step_fused(self._fq, x, None if sample_out is not None else a_tanh, self._eps_pi,
                                        self.log_c_alpha, q_out=self._pi_q, defer=fold, subset=sub if E != 2 else None,
                                        sample_out=sample_out, offline=offline)
        else:
            c_qs = self._fq._launch_forward(x, a_tanh, out=self._pi_q)                   # [E, B, 1]
            # objective gradients formed on chip: dL/dq inside the Q backward (from the value table), dL/dlogp =
            # alpha / B inside the sampling backward; the logged statistics are computed on demand
            g_a = self._fq.backward_policy_q(x, a_tanh, c_qs.view(E, B), sub if self.ensemble_q_sample != E else None,
                                             self.ensemble_q_sample)                    # [E, B, A]
            # sampling backward (sums the members' action gradients) + policy backward in one launch
            self._fpi.backward_policy_sample(x, self._eps_pi, g_a, self.log_c_alpha, defer=fold, offline=offline)
        if fold:
            self._fpi.adam_partials(opt)
            return
        if self._dist is not None:
            self._dist.all_reduce_grads(self._params.grad, *self._params.span('policy'))
        opt.step()

    def _train_policy(self, obs_list, state, action, mu_d_policy_probs, ls=None):
        dsum, E = self.d_action_summed_size, self.ensemble_q_num
        offline = self.offline_enabled and self.offline_loss
        if self._stock_c_only():
            return self._train_policy_stock(state, ls, offline=action[..., dsum:] if offline else None)
        if self._discrete_fused(state.shape[0]):
            # pure-discrete: the critics only supply values; objective, entropy statistic and d loss / d logits from one
            # launch; back-propagation starts at the logits
            logits = self._discrete_logits(state, obs_list)
            with torch.no_grad():
                d_qs = self._d_q_heads(False, state, obs_list, action[..., dsum:])
            sub = self._subsets['pi_d']
            self.noise.subset_(sub, E)
            _, grad_logits = self._discrete_grad_buffers(state.shape[0])
            native.discrete_policy_loss_grad(self._branches, logits.detach(), d_qs, sub, self.ensemble_q_sample,
                                             mu_d_policy_probs, self.log_d_alpha, self.d_policy_entropy_penalty,
                                             self._stats['loss_policy'], grad_logits, self._stats['d_entropy'])
            pi_inputs = list(self.model_policy.parameters())
            with direct_param_grads(only=pi_inputs):
                torch.autograd.backward([logits], [grad_logits], inputs=pi_inputs)
            self.optimizer_policy.step()
            return
        if self._hybrid_fused(state.shape[0]):
            # hybrid: the critics only supply values (the discrete ones at the stored continuous action, the continuous ones
            # at the sample); objective, both entropy statistics and d loss / d (logits, logp, continuous values) from one
            # launch; back-propagation starts there, restricted to the policy.  Draws in the eager order: pi_d, noise, pi_c
            logits, loc, scale = self._hybrid_heads(state, obs_list)
            with torch.no_grad():
                d_qs = [q(state, action[..., dsum:], obs_list)[0] for q in self.model_q_list]
            sub_d = self._subsets['pi_d']
            self.noise.subset_(sub_d, E)
            self.noise.normal_(self._eps_pi)
            a_tanh, logp = squash_sample(loc, scale, self._eps_pi)
            c_qs = torch.stack([q(state, a_tanh, obs_list)[1] for q in self.model_q_list]).squeeze(-1)   # [E, B]
            sub_c = self._subsets['pi_c']
            self.noise.subset_(sub_c, E)
            buf = self._hybrid_buffers(state.shape[0])
            native.hybrid_policy_loss_grad(
                self._branches, logits.detach(), d_qs, sub_d, mu_d_policy_probs, self.log_d_alpha,
                self.d_policy_entropy_penalty, logp.detach(), c_qs.detach().contiguous(),
                sub_c if self.ensemble_q_sample != E else None, self.ensemble_q_sample, self.log_c_alpha, scale.detach(),
                self._stats['loss_policy'], buf['grad_logits'], buf['grad_logp'], buf['grad_cq'], self._stats['d_entropy'],
                self._stats['c_entropy'])
            pi_inputs = list(self.model_policy.parameters())
            with direct_param_grads(only=pi_inputs):
                torch.autograd.backward([logits, logp, c_qs], [buf['grad_logits'], buf['grad_logp'], buf['grad_cq']],
                                        inputs=pi_inputs)
            self.optimizer_policy.step()
            return
        d_policy, c_policy, loc, scale, plain = self._policy(state, obs_list)
        loss_d = loss_c = None
        with torch.no_grad():
            d_alpha = torch.exp(self.log_d_alpha) if self.d_action_sizes else None
            c_alpha = torch.exp(self.log_c_alpha) if self.c_action_size else None

        if self.d_action_sizes and self.discrete_dqn_like and not self.c_action_size:
            with torch.no_grad():   # nothing to optimise (1905); keep the logged entropy
                self._stats['d_entropy'].copy_(torch.mean(d_policy.entropy().sum(-1) / self.d_action_branch_size))
            return
        if self.d_action_sizes and not self.discrete_dqn_like:
            probs = d_policy.probs
            c_action = action[..., dsum:]
            if self.c_action_size:
                d_qs = torch.stack([q(state, c_action, obs_list)[0] for q in self.model_q_list])
            else:
                d_qs = torch.stack(self._d_q_heads(False, state, obs_list, c_action))
            sub = self._subsets['pi_d']
            self.noise.subset_(sub, E)
            mean_q = d_qs.index_select(0, sub.long()).mean(0)
            inner = d_alpha * torch.log(probs.clamp(min=1e-8)) - mean_q.detach()
            loss_d = torch.sum(probs * inner, dim=1, keepdim=True) / self.d_action_branch_size
            mu_ent = -torch.sum(mu_d_policy_probs * torch.log(mu_d_policy_probs.clamp(min=1e-8)), dim=-1) \
                / self.d_action_branch_size
            pi_ent = d_policy.entropy().sum(-1) / self.d_action_branch_size
            loss_d = loss_d + self.d_policy_entropy_penalty * (torch.pow(mu_ent - pi_ent, 2.) / 2.).unsqueeze(-1)

        # restricted to the policy: its parameters (and the fused policy's anchor); the Q ensemble only passes the
        # action gradient through (param_grads=False), so the direct accumulation reaches the policy alone
        pi_inputs = list(self.model_policy.parameters()) + ([self._fpi._anchor] if self._fpi is not None else [])
        if self.c_action_size and not self.d_action_sizes and plain and (not offline or self._offline_plain()):
            # continuous-only fast path: objective, its gradients and the entropy statistic from one
            # launch; back-propagation starts at (logp, q) with the kernel-produced gradients
            self.noise.normal_(self._eps_pi)
            if self._ls is not None:
                a_tanh, logp = squash_sample_ls(self._ls, self._eps_pi)
            else:
                a_tanh, logp = squash_sample(loc, scale, self._eps_pi)
            c_qs = self._c_q_values(False, state, a_tanh, obs_list, param_grads=False)        # [E, B]
            sub = self._subsets['pi_c']
            self.noise.subset_(sub, E)
            native.policy_loss_fwd_bwd(logp.detach(), c_qs.detach().contiguous(),
                                       sub if self.ensemble_q_sample != E else None, self.ensemble_q_sample,
                                       self.log_c_alpha, scale.detach(), self._stats['loss_policy'],
                                       self._grad_logp, self._grad_q, self._stats['c_entropy'])
            heads, grads = [logp, c_qs], [self._grad_logp, self._grad_q]
            if offline:
                # the offline loss: + mean_b sum_d (u - stored action)^2 on the pre-tanh sample u (reference 1899-1900),
                # value into the logged objective and gradient at u from one more launch
                u = loc + scale * self._eps_pi
                ls_rows = (self._ls if self._ls is not None else torch.cat([loc, scale], -1)).detach()
                grad_u = torch.empty_like(self._eps_pi)
                native.policy_offline_term(ls_rows, self._eps_pi, action[..., dsum:], self._stats['loss_policy'], grad_u)
                heads, grads = heads + [u], grads + [grad_u]
            with direct_param_grads(only=pi_inputs):
                torch.autograd.backward(heads, grads, inputs=pi_inputs)
            if self._dist is not None:
                self._dist.all_reduce_grads(self._params.grad, *self._params.span('policy'))
            self.optimizer_policy.step()
            return

        if self.c_action_size:
            self.noise.normal_(self._eps_pi)
            if plain:
                a_tanh, logp = squash_sample(loc, scale, self._eps_pi)
                logp = logp.unsqueeze(-1)
            else:
                sampled = self._rsample(c_policy, self._eps_pi)
                a_tanh = torch.tanh(sampled)
                logp = sum_log_prob(squash_correction_log_prob(c_policy, sampled), keepdim=True)
            if self.d_action_sizes:
                c_qs = torch.stack([q(state, a_tanh, obs_list)[1] for q in self.model_q_list])   # [E, B, 1]
            else:   # gradient flows to the action only (the update is restricted to the policy)
                c_qs = self._c_q_values(False, state, a_tanh, obs_list, param_grads=False).unsqueeze(-1)
            sub = self._subsets['pi_c']
            self.noise.subset_(sub, E)
            if self.ensemble_q_sample != E:
                c_qs = c_qs.index_select(0, sub.long())
            loss_c = c_alpha * logp - c_qs.min(dim=0)[0]
            if self.offline_enabled and self.offline_loss:
                loss_c = loss_c + functional.mse_loss(torch.atanh(a_tanh.clamp(-0.999999, 0.999999)), action[..., dsum:],
                                                      reduction='none').sum(-1, keepdim=True)

        loss = torch.mean(loss_c if loss_d is None else (loss_d if loss_c is None else loss_d + loss_c))
        with direct_param_grads(only=pi_inputs):
            loss.backward(inputs=pi_inputs)
        if self._dist is not None:
            self._dist.all_reduce_grads(self._params.grad, *self._params.span('policy'))
        self.optimizer_policy.step()
        with torch.no_grad():
            self._stats['loss_policy'].copy_(loss.detach())
            if self.d_action_sizes:
                self._stats['d_entropy'].copy_(torch.mean(d_policy.entropy().sum(-1) / self.d_action_branch_size))
            if self.c_action_size:
                if plain:   # Normal entropy = 1/2 + 1/2 log(2 pi) + log(scale)
                    self._stats['c_entropy'].copy_(torch.mean((torch.log(scale) + 1.4189385332046727).sum(-1)))
                else:
                    self._stats['c_entropy'].copy_(torch.mean(sum_entropy(c_policy.entropy())))

    def _train_alpha(self, obs_list, state, ls=None, logp=None):
        """`ls`: the (updated) policy's [B, 2A] (loc | scale) output for `state`, if the caller has it;
        `logp`: log pi of an action already drawn from it with `self._eps_alpha`."""
        if self._discrete_fused(state.shape[0]):
            # pure-discrete: dL/dlog_d_alpha = mean_b (1/K) sum_j p_j (-cl(p_j) - target_j) straight into its gradient slot
            # (log_c_alpha's slot keeps the zero the step's prologue wrote, as after the eager backward)
            with torch.no_grad():
                seg0 = self._params.segments['alpha'][0]
                native.discrete_alpha_grad(self._branches, self._discrete_logits(state, obs_list), self.target_d_alpha,
                                           self._params.grad[seg0:seg0 + 1])
            self.optimizer_alpha.step()
            return
        if ls is None and logp is None and self._hybrid_fused(state.shape[0]):
            # hybrid: both temperature gradients straight into their slots [log_d_alpha, log_c_alpha] from one launch, the
            # continuous one on log pi of a fresh sample
            with torch.no_grad():
                logits, loc, scale = self._hybrid_heads(state, obs_list)
                self.noise.normal_(self._eps_alpha)
                loc, scale = loc.contiguous(), scale.contiguous()
                scratch = torch.empty_like(loc)
                logp = torch.empty(loc.shape[:-1], dtype=torch.float32, device=self.device)
                native.squash_sample_fwd(loc, scale, self._eps_alpha, scratch, logp)
                seg0 = self._params.segments['alpha'][0]
                native.hybrid_alpha_grad(self._branches, logits, self.target_d_alpha, logp,
                                         self.target_c_alpha * -float(self.c_action_size),
                                         self._params.grad[seg0:seg0 + 2])
            self.optimizer_alpha.step()
            return
        with torch.no_grad():
            if ls is not None:
                A = self.c_action_size
                d_policy = c_policy = None
                loc, scale, plain = ls[..., :A], ls[..., A:], True
            else:
                d_policy, c_policy, loc, scale, plain = self._policy(state, obs_list)
        loss_d = loss_c = None
        if self.c_action_size and not self.d_action_sizes and plain:
            # continuous-only fast path: dL/dlog_alpha = mean(-logp) - target straight into its gradient slot
            with torch.no_grad():
                if logp is None:
                    self.noise.normal_(self._eps_alpha)
                    scratch = torch.empty(loc.shape, dtype=torch.float32, device=self.device)
                    logp = torch.empty(loc.shape[:-1], dtype=torch.float32, device=self.device)
                    native.squash_sample_fwd(loc, scale, self._eps_alpha, scratch, logp)
                seg0, seg1 = self._params.segments['alpha']
                target = self.target_c_alpha * -float(self.c_action_size)
                opt = self.optimizer_alpha
                if self._dist is None and (opt.start, opt.stop) == (seg0, seg1):
                    g = self._params                       # gradient + Adam in one launch
                    # the last optimizer launch of the step when no further head trains: it also
                    # advances the shared Adam step counter
                    last = self.curiosity is None and not self.use_rnd
                    native.alpha_adam_step(logp, target, 1, g.flat[seg0:seg1], g.grad[seg0:seg1],
                                           opt.exp_avg[seg0:seg1], opt.exp_avg_sq[seg0:seg1], opt.lr,
                                           opt.betas[0], opt.betas[1], opt.eps, opt.steps_done,
                                           advance_counter=last)
                    self._counter_advanced = last
                    return
                native.alpha_grad(logp, target, self._params.grad[seg0 + 1:seg0 + 2])   # [log_d_alpha, log_c_alpha]
            if self._dist is not None:
                self._dist.all_reduce_grads(self._params.grad, *self._params.span('alpha'))
            self.optimizer_alpha.step()
            return
        if self.d_action_sizes and not self.discrete_dqn_like:
            probs = d_policy.probs
            inner = self.log_d_alpha * (-torch.log(probs.clamp(min=1e-8)) - self.target_d_alpha)
            loss_d = torch.sum(probs * inner, dim=1, keepdim=True) / self.d_action_branch_size
        if self.c_action_size:
            self.noise.normal_(self._eps_alpha)
            with torch.no_grad():
                if plain:
                    loc, scale = loc.contiguous(), scale.contiguous()
                    scratch = torch.empty_like(loc)
                    logp = torch.empty(loc.shape[:-1], dtype=torch.float32, device=self.device)
                    native.squash_sample_fwd(loc, scale, self._eps_alpha, scratch, logp)
                    logp = logp.unsqueeze(-1)
                    valid = float(self.c_action_size)
                else:
                    sampled = self._eps_alpha * c_policy.scale + c_policy.loc
                    if hasattr(c_policy, 'padding_mask'):
                        sampled[..., c_policy.padding_mask] = 0.
                    lp = squash_correction_log_prob(c_policy, sampled)
                    valid = torch.sum(lp != torch.inf, dim=-1, keepdim=True)
                    logp = sum_log_prob(lp, keepdim=True)
            loss_c = self.log_c_alpha * (-logp - self.target_c_alpha * -valid)
        loss = torch.mean(loss_c if loss_d is None else (loss_d if loss_c is None else loss_d + loss_c))
        loss.backward(inputs=[self.log_d_alpha, self.log_c_alpha])
        if self._dist is not None:
            self._dist.all_reduce_grads(self._params.grad, *self._params.span('alpha'))
        self.optimizer_alpha.step()

    def _alpha_sidecar(self, logp):
        """the continuous-only temperature step (`_train_alpha`'s one-launch form) as a sidecar job, or None when
        that form does not apply (an optimizer over more than the two temperatures).  Data parallel: the caller
        averages `logp` over the ranks between the launch that writes it and the launch that hosts the job
        (`_alpha_logp_over_ranks`): the gradient mean_b(-logp_b) - target is linear in it, so the job then applies the
        rank-averaged gradient — one collective on B floats instead of gradient launch + collective + Adam launch"""
        seg0, seg1 = self._params.segments['alpha']
        opt = self.optimizer_alpha
        if (opt.start, opt.stop) != (seg0, seg1) or self.d_action_sizes:
            return None
        g = self._params
        last = self.curiosity is None and not self.use_rnd      # the step's last optimizer launch advances the counter
        self._counter_advanced = last
        return native.sidecar_alpha_adam(logp, self.target_c_alpha * -float(self.c_action_size), 1, g.flat[seg0:seg1],
                                         g.grad[seg0:seg1], opt.exp_avg[seg0:seg1], opt.exp_avg_sq[seg0:seg1], opt.lr,
                                         opt.betas[0], opt.betas[1], opt.eps, opt.steps_done, advance_counter=last)

    def _alpha_logp_over_ranks(self, logp) -> None:
        if self._dist is not None:
            self._dist.all_reduce_grads(logp, 0, logp.numel())

    def _train_curiosity(self, n_padding_masks, nx_states, n_actions):
        # the reference differentiates w.r.t. the model's parameters only (`backward(inputs=parameters)`,
        # sac_base.py:1951-1976): same gradients from detached inputs, which lets the fused stack add its
        # parameter gradients where they live
        nx_states, n_actions = nx_states.detach(), n_actions.detach()
        n_states, next_n_states = nx_states[:, :-1], nx_states[:, 1:]
        if self.curiosity == CURIOSITY.FORWARD:
            pred, target = self.model_forward_dynamic(n_states, n_actions), next_n_states
        else:
            pred, target = self.model_inverse_dynamic(n_states, next_n_states), n_actions
        _masked_mse_backward(pred, target, n_padding_masks, self._stats['loss_curiosity'], fused=self._fused_curiosity)
        if self._dist is not None:
            self._dist.all_reduce_grads(self._params.grad, *self._params.span('curiosity'))
        self.optimizer_curiosity.step()

    @torch.no_grad()
    def _get_td_error(self, n_last_masks, n_padding_masks, nx_obses_list, state, nx_target_states, nx_actions,
                      n_rewards, n_dones, n_mu_probs, ls=None, sample=None, stored_pi=None, c_q=None, q_table=None, *,
                      sidecars=None, pending_alpha=None, td_update=None):
        """mean_e |Q_e(s0, a0) - y(target states)| -> (self._td_error [B], the launch that formed it was the priority
        update too) (reference 2182-2245).  `ls` .. `q_table`: see `_get_y`; the keywords: see `_launch_return`."""
        dsum = self.d_action_summed_size
        obs_list = [o[:, 0] for o in nx_obses_list]
        action = nx_actions[:, 0]
        d_action, c_action = action[..., :dsum], action[..., dsum:]
        if c_q is None and self._discrete_fused(state.shape[0]):
            # pure-discrete: the return's launch writes mean_e |(1/K) sum_j a_j q_e - y| itself
            assert not sidecars and pending_alpha is None and td_update is None
            heads = self._d_q_heads(False, state, obs_list, c_action)
            self._get_y(n_last_masks, n_padding_masks, nx_obses_list, nx_target_states, nx_actions, n_rewards, n_dones,
                        n_mu_probs, eps_buf=self._eps_td, subset_prefix='td', y_out=self._y_td_buf, td_out=self._td_error,
                        d_q_online=heads)
            return self._td_error, False
        if c_q is None and ls is None and sample is None and self._hybrid_fused(state.shape[0]):
            # hybrid: the return's launch writes mean_e (|(1/K) sum_j a_j q_e - d_y| + |c_q_e - c_y|) itself
            assert not sidecars and pending_alpha is None and td_update is None
            q_list = [q(state, c_action, obs_list) for q in self.model_q_list]
            c_q = torch.stack([q[1] for q in q_list]).squeeze(-1).contiguous()
            self._get_y(n_last_masks, n_padding_masks, nx_obses_list, nx_target_states, nx_actions, n_rewards, n_dones,
                        n_mu_probs, eps_buf=self._eps_td, subset_prefix='td', y_out=self._y_td_buf, td_out=self._td_error,
                        q_online=c_q, d_q_online=[q[0] for q in q_list])
            return self._td_error, False
        if c_q is None and self._dqn_fused(state.shape[0]):
            # DQN-like: the return's launch writes mean_e |(1/K) sum_j a_j q_e - y| itself
            assert not sidecars and pending_alpha is None and td_update is None
            heads = self._d_q_heads(False, state, obs_list, c_action)
            ret = self._dqn_target_job(n_last_masks, n_padding_masks, nx_obses_list, nx_target_states, nx_actions,
                                       n_rewards, n_dones, subset_prefix='td', y_out=self._y_td_buf, q_online=heads,
                                       td_out=self._td_error)
            native.dqn_return(*ret.args)
            del ret
            return self._td_error, False
        q_list = None
        if c_q is not None:
            pass                  # [E, B] online Q of (s0, a0), already computed by the caller
        elif self.d_action_sizes and not self.c_action_size:
            q_list = [(h, None) for h in self._d_q_heads(False, state, obs_list, c_action)]
        elif self.d_action_sizes:
            q_list = [q(state, c_action, obs_list) for q in self.model_q_list]
            c_q = torch.stack([q[1] for q in q_list]).squeeze(-1).contiguous()
        else:
            c_q = self._c_q_values(False, state, c_action, obs_list).contiguous()
        fused_td = bool(self.c_action_size) and not self.d_action_sizes
        d_y, c_y, ret = self._get_y(n_last_masks, n_padding_masks, nx_obses_list, nx_target_states, nx_actions,
                                    n_rewards, n_dones, n_mu_probs, eps_buf=self._eps_td, subset_prefix='td',
                                    y_out=self._y_td_buf, q_online=c_q if fused_td else None, td_out=self._td_error,
                                    ls=ls, sample=sample, stored_pi=stored_pi, q_table=q_table, launch=False)
        if fused_td:    # (only then are there riders: they come from the stock continuous-only chain)
            return self._td_error, self._launch_return(ret, sidecars=sidecars, pending_alpha=pending_alpha,
                                                       td_update=td_update)
        assert not sidecars and pending_alpha is None and td_update is None
        if ret is not None:
            self._launch_return(ret)
        err = torch.zeros((self.ensemble_q_num, state.shape[0], 1), device=self.device)
        if self.d_action_sizes:
            d_q = torch.stack([torch.sum(d_action * q[0], dim=-1, keepdim=True) / self.d_action_branch_size
                               for q in q_list])
            err = err + torch.abs(d_q - d_y)
        if self.c_action_size:
            err = err + torch.abs(c_q.unsqueeze(-1) - c_y)
        self._td_error.copy_(err.mean(dim=0).reshape(-1))
        return self._td_error, False

    # ==========================================================================================
    # episode ingress (reference sac_base.py:2303-2396)
    # ==========================================================================================
    def put_episode(self, ep_indexes, ep_obses_list, ep_actions, ep_rewards, ep_dones, ep_probs,
                    ep_pre_seq_hidden_states) -> None:
        """Reference sac_base.py:2303-2396.  NumPy arrays (the reference's callers) or tensors already in HBM
        (the device-resident `AgentManager`): the latter go slab -> ring without touching the host."""
        if ep_indexes.shape[1] < self.n_step:
            return
        if isinstance(ep_indexes, torch.Tensor):
            assert ep_indexes.dtype == torch.int32
            last = ep_indexes == -1
            last[:, -1] = True
            obs_dev = [o[0] for o in ep_obses_list]
        else:
            assert ep_indexes.dtype == np.int32
            last = np.zeros_like(ep_indexes, dtype=bool)
            last[:, -1] = True
            last[ep_indexes == -1] = True
            obs_dev = None
        if not self.use_replay_buffer:
            # (the reference updates the normalizer only on the replay path: `_fill_replay_buffer`)
            self.batch_buffer.put_episode(ep_indexes, last, ep_obses_list, ep_actions, ep_rewards, ep_dones, ep_probs,
                                          ep_pre_seq_hidden_states)
            return
        rows = {'index': ep_indexes[0], 'last_mask': last[0],
                **{f'obs_{name}': o[0] for name, o in zip(self.obs_names, ep_obses_list)},
                'action': ep_actions[0], 'reward': ep_rewards[0], 'done': ep_dones[0],
                'mu_prob': ep_probs[0], 'pre_seq_hidden_state': ep_pre_seq_hidden_states[0]}
        if self.use_normalization:
            ep_obs = obs_dev if obs_dev is not None else [torch.from_numpy(o[0]).to(self.device) for o in ep_obses_list]
            if self.normalizer is not None:
                self.normalizer.update(ep_obs)       # one launch for all observations
            else:
                self._update_normalizer(ep_obs)
        self.replay_buffer.add(rows, ignore_size=1)

    # ==========================================================================================
    # the step
    # ==========================================================================================
    def _device_step(self) -> None:
        # the representation passes of a step see the same window buffers: attention blocks build their index /
        # padding / attention masks once per step (nn_models.layers.seq_layers.step_mask_cache)
        with step_mask_cache() if self.seq_encoder == SEQ_ENCODER.ATTN else contextlib.nullcontext():
            self._device_step_body()

    def _device_step_body(self) -> None:
        """Everything one `train()` does on the device, without a single host synchronisation
        (reference `_sample_from_replay_buffer` 2398-2494, `_train` 2027-2126, write-backs 2558-2605).
        Reads / writes only static buffers, so it can be captured and replayed as a hipGraph.  Phases:
          _step_sample            prologue (Polyak, draws) + PER sample + window gather -> views of the static batch
          _step_rep_and_q         representation passes (online, target), Q step, states under the updated representation
          _step_policy            policy step
          _step_after_policy_*    stock networks: the UPDATED policy over the window -> new behaviour probabilities, the
                                  TD target's sample, the temperature step's sample (one launch, or the chain it replaces)
          _step_temperature_and_aux  temperature step (unless a sidecar took it), curiosity / RND
          _step_write_backs       TD error -> priorities, mu-probability and hidden-state rows"""
        self._counter_advanced = False
        w = self._step_sample()
        self._step_rep_and_q(w)
        self._join_head_gather()       # (taken by the first network launch, or issued in front of it: never still pending)
        self._step_policy(w)
        post = _AfterPolicy()
        if not self.use_replay_buffer:
            # batch mode (reference train 2536-2539): no TD error, no priorities, no mu-probability / hidden-state
            # write-back — only the temperature step follows the policy step
            self._step_temperature_and_aux(w, post)
            if not self._counter_advanced:
                self._opt_steps.add_(1)
            self.batch_buffer.advance_head()     # (every launch that read the head is behind us)
            return
        self._join_lookahead()       # (everything below may write priorities / replay rows)
        if w.stock and self.use_n_step_is:
            with torch.no_grad():
                if not self._step_after_policy_one_launch(w, post):
                    self._step_after_policy_chain(w, post)
        self._step_temperature_and_aux(w, post)
        self._step_write_backs(w, post)
        if not self._counter_advanced:
            self._opt_steps.add_(1)

    def _join_lookahead(self) -> None:
        if self._la_gather is not None:      # no launch hosted the next batch's gather: on its own, before any write-back
            self._la_gather = None
            self.replay_buffer.gather_next_now()

    def _head_gather_plan(self, rb, build=False):
        """-> `rb.head_gather` where the step's first network launch is the stock one-launch forward chain on the gathered
        vector observation itself (parameter-free representation: the state IS that buffer), else None.  The answer is kept
        per static set (`rb._gather_keys`): `train()` pays one identity test per call, `build` (host time, a blocking copy)
        happens where a set is new — never on a replayed step, never inside a capture."""
        cached = self._head_plan_cache
        if cached is not None and cached[0] is rb._gather_keys:
            return cached[1]
        if not build:
            return None
        plan = None
        # (no burn-in: the window views are then the whole buffers, nothing copies them in front of the launch; a batch of
        # more than 256 rows with deferred weights keeps `window_gather_pad_w`)
        weights = self._defer_is_weights
        # (a normalized learner: the first network launch would read RAW rows from the ring — the gather runs on its own,
        # the whiten launch follows and the stock chain reads the whitened buffer)
        if (self._head_gather_sidecar and self._lookahead == 0 and self.burn_in_step == 0 and self._dist is None
                and self.normalizer is None and self._stock_c_only()
                and type(self.model_rep) is ModelSimpleRep and self.optimizer_rep is None
                and self.clip_epsilon > 0 and self.siamese is None and not self.use_prediction
                and not self._wide_critics and len(self.obs_names) == 1 and not (weights and rb.batch_size > 256)):
            plan = rb.head_gather(f'obs_{self.obs_names[0]}', build=True, weights=weights)
        self._head_plan_cache = (rb._gather_keys, plan)
        return plan

    def _join_head_gather(self) -> None:
        if self._head_gather is not None:    # no launch took the step's gather as a rider: on its own, before its first reader
            self._head_gather = None
            self.replay_buffer.gather_now(weights=self._head_gather_w)

    def _take_la_gather(self):
        """-> the pending gather of the NEXT batch as a sidecar list for a launch that reads nothing of it, or None"""
        sc, self._la_gather = self._la_gather, None
        return None if sc is None else [sc]

    def _step_sample(self):
        """-> the step's window views (`_Window`): [B, L] tensors are `bnx_*`, their first L - 1 rows `bn_*`"""
        rb, b = getattr(self, 'replay_buffer', None), self.burn_in_step
        # Polyak of every step rides in the step's first launch, together with every uniform / Gaussian draw and
        # ensemble subset of the step (recorded test noise: a plain Polyak launch, draws injected by the test)
        polyak = None
        if self.update_target_per_step == 1 and self._polyak_len > 0:
            polyak = (self._target_params.flat[:self._polyak_len], self._params.flat[:self._polyak_len], self.tau)
        zero = None if self._grads_overwrite else self._params.grad
        if not self.use_replay_buffer:
            # batch mode: no PER draws; the oldest queued batch -> the static batch (one launch)
            self.noise.begin_step(self._opt_steps, None, self._eps_all, self._subsets_all, self.ensemble_q_num,
                                  polyak=polyak, zero=zero)
            self.batch_buffer.gather_into_static()
            return self._window_views(self.batch_buffer._batch, None, None, None)
        if self._lookahead:
            # the batch this step trains on was drawn during the previous step (`train` swapped the sets); the NEXT one
            # is drawn now, from the tree and the rows as the previous step left them, before this step's first write to
            # the replay
            sampled = False
            if self._use_sidecars:
                # the prologue launch hosts the NEXT batch's tree walk (its sampler workgroup), as in the plain schedule
                rb.swap_sets()
                try:
                    sampled = self.noise.begin_step_with_sample(self._opt_steps, rb, self._eps_all, self._subsets_all,
                                                                self.ensemble_q_num, polyak=polyak, zero=zero)
                finally:
                    rb.swap_sets()
            if not sampled:
                self.noise.begin_step(self._opt_steps, rb.next_uniforms() if rb.uniform_source is self.noise else None,
                                      self._eps_all, self._subsets_all, self.ensemble_q_num, polyak=polyak, zero=zero)
            if sampled and self._la_gather_sidecar:
                # ... and its window gather rides as extra workgroups of the step's first policy / critic launch
                # (`_take_la_gather`; `_join_lookahead` runs it on its own if no launch took it)
                self._la_gather = rb.next_gather_sidecar()
            else:
                rb.sample_next_into_static(sampled=sampled)      # same launches, in line
        else:
            # ... and the sampler of the batch it draws: one launch for K1 + K2 + K5
            # (where the step's first network launch will carry the gather, the IS weights of a one-workgroup batch ride
            # there too: the sampler leaves them out — `defer_small`)
            head = self._head_gather_plan(rb)
            sampled = self._use_sidecars and self.noise.begin_step_with_sample(
                self._opt_steps, rb, self._eps_all, self._subsets_all, self.ensemble_q_num, polyak=polyak, zero=zero,
                defer_weights=self._defer_is_weights, defer_small=head is not None)
            if not sampled:
                self.noise.begin_step(self._opt_steps, rb._u if rb.uniform_source is self.noise else None, self._eps_all,
                                      self._subsets_all, self.ensemble_q_num, polyak=polyak, zero=zero)
            # the gather rides in the step's first network launch where that launch can read its rows from the ring
            # (`_train_rep_q_stock` takes it; `_join_head_gather` issues it on its own in front of any other reader)
            self._head_gather_w = sampled == 3
            self._head_gather = head if head is not None and ('sidecar_w' if sampled == 3 else 'sidecar') in head else None
            if not sampled:
                self._head_gather = None
            rb.sample_into_static(sampled=sampled, gather=self._head_gather is None)
        derived = rb.derived if rb.derived is not None and rb.sharded is None else None
        return self._window_views(rb._batch, rb._ids, rb._w.unsqueeze(-1) if self.use_priority else None, derived,
                                  rb.joint_pre_action)

    def _window_views(self, batch, ids, priority_is, derived, joint_pre_action=None):
        b = self.burn_in_step
        w = _Window()
        w.ids = ids
        w.priority_is = priority_is
        w.bnx_obses_list = [batch[f'obs_{name}'] for name in self.obs_names]
        w.bnx_actions, w.bnx_pad = batch['action'], batch['padding_mask']
        w.bn_indexes, w.bn_last, w.bn_pad = batch['index'][:, :-1], batch['last_mask'][:, :-1], w.bnx_pad[:, :-1]
        w.bn_actions, w.bn_rewards, w.bn_dones = w.bnx_actions[:, :-1], batch['reward'][:, :-1], batch['done'][:, :-1]
        w.bn_mu_probs = batch['mu_prob'][:, :-1]
        w.bnx_hidden = batch['pre_seq_hidden_state']
        w.nx_obs = [o[:, b:] for o in w.bnx_obses_list]
        w.obs_b = [o[:, b] for o in w.bnx_obses_list]
        w.stock = self._stock_c_only()
        w.rep_trainable = self.optimizer_rep is not None
        self.noise.prefill(self._eps_all)          # (torch fallback: one launch for all Gaussian draws)
        rep_obs = w.bnx_obses_list
        if self.normalizer is not None:
            # the step's ONE whitening, behind the batch's gather and with the statistics of train time: all window
            # observations -> static buffers of their shapes.  Every representation pass of the step reads these
            # (`_l_states_whitened`); whatever else reads observations (`w.nx_obs`, `w.obs_b`) keeps the raw buffers
            rep_obs = self.normalizer.whiten(w.bnx_obses_list, static=True)
        if type(self.model_rep) is ModelSimpleRep:
            # the stock concatenation rep ignores index / mask / previous actions: do not build them
            w.rep_in = (None, None, rep_obs, None, w.bnx_hidden)
        else:
            if derived is not None:
                # (the gather delivered them as derived keys of its launch: no `asac_window_aux`)
                d = derived
                bnx_indexes, bnx_padding_masks, bnx_pre_actions = d['index_x'], d['padding_mask_x'], d['pre_action']
            else:
                bnx_indexes, bnx_padding_masks, bnx_pre_actions = self.get_bnx_data(
                    w.bn_indexes, w.bn_pad, w.bn_actions, pre_action_out=joint_pre_action)
            w.rep_in = (bnx_indexes, bnx_padding_masks, rep_obs, bnx_pre_actions, w.bnx_hidden)
        return w

    def _step_rep_and_q(self, w) -> None:
        """reference `_train` 2066-2103: online and target representation over the window, `_train_rep_q`, the states
        again under the updated representation -> w.bnx_states, w.bnx_target_states, w.next_hidden"""
        b = self.burn_in_step
        cat_mode = self._cat_mode if self._cat_mode is not None else contextlib.nullcontext
        with_aux = self.siamese is not None or self.use_prediction
        # A representation without a sequence encoder maps every step on its own (it is handed single steps when
        # acting), and the Q loss reads the state of ONE window position — everything else of the window only feeds
        # detached targets.  The differentiable pass then covers that position's rows alone (B of B L frames: the
        # backward of a convolution stack shrinks L-fold) beside a no-grad pass over the window.
        # (where the pass in front of the update already covers only a few positions — `from_b` below, n + 1 <= 8 — the
        # extra forward's small-launch floors cost more than the backward over those few positions saves: cfg4, n + 1 = 4,
        # 2 755 with it against 2 787 steps/s without)
        one_position = (self._rep_grad_one_position and self.seq_encoder is None and w.rep_trainable and not with_aux
                        and type(self.model_rep) is not ModelSimpleRep and w.bnx_actions.shape[1] > 1
                        and not (self._rep_from_burn_in and b > 0 and self.n_step + 1 <= 8))
        # ... and the burn-in positions of the window feed nothing before the update (a sequence encoder would carry them
        # forward; here states[:, b:] is all `_train_rep_q`, the return and the TD error read): the two passes in front of
        # the update run on the positions from b on — (n + 1) / L of the frames, read in place (`asac_conv2_forward_windows`)
        from_b = (self._rep_from_burn_in and self.seq_encoder is None and b > 0 and w.rep_trainable
                  and type(self.model_rep) is not ModelSimpleRep)     # (a fixed representation's one pass serves the whole step)
        rep_in, pb = w.rep_in, b
        # (a normalized learner's window is whitened already: its passes go around `get_l_states`' whitening)
        l_states = self.get_l_states if self.normalizer is None else self._l_states_whitened
        if from_b:
            tail = lambda x: None if x is None else x[:, b:]  # noqa: E731
            idx, pad, obs, pre, hidden = w.rep_in
            rep_in, pb = (tail(idx), tail(pad), [o[:, b:] for o in obs], tail(pre), tail(hidden)), 0
        with (self._rep_twin if self._rep_twin else contextlib.nullcontext()), cat_mode():
            with torch.no_grad() if one_position else contextlib.nullcontext():
                bnx_states, next_hidden = l_states(*rep_in, is_target=False)
            with torch.no_grad():
                w.bnx_target_states, _ = l_states(*rep_in, is_target=True)
        w.nx_target_states = w.bnx_target_states[:, pb:]
        state_base = (bnx_states, pb)
        if one_position:
            at = lambda x: None if x is None else x[:, b:b + 1]  # noqa: E731
            idx, pad, obs, pre, hidden = w.rep_in
            with cat_mode():
                state_b, _ = l_states(at(idx), at(pad), [o[:, b:b + 1] for o in obs], at(pre), at(hidden), is_target=False)
            state_base = (state_b, 0)
        aux = None
        if with_aux:
            aux = dict(n_indexes=w.bn_indexes[:, b:],
                       n_pre_actions=w.bn_actions[:, b - 1:-1] if b > 0 else w.bn_actions[:, 0:0],
                       n_pre_seq_hidden_states=w.bnx_hidden[:, b:-1], nx_target_states=w.nx_target_states)
        self._train_rep_q(w.bn_last[:, b:], w.bn_pad[:, b:], w.nx_obs, time_slice(bnx_states, pb), w.bnx_actions[:, b:],
                          w.bn_rewards[:, b:], w.bn_dones[:, b:], w.bn_mu_probs[:, b:], w.priority_is, aux,
                          policy_sample=w.stock and not w.rep_trainable,
                          state_base=state_base)
        if w.rep_trainable:   # states under the updated representation (reference 2097-2103)
            with torch.no_grad(), cat_mode():
                w.bnx_states, w.next_hidden = l_states(*w.rep_in, is_target=False)
        else:
            w.bnx_states, w.next_hidden = bnx_states.detach(), next_hidden.detach()

    def _step_policy(self, w) -> None:
        b = self.burn_in_step
        w.state_b = w.bnx_states[:, b]
        # the target computation already ran the (still unchanged) policy on this state: reuse its output
        ls_b = self._ls_y[:, 0] if (w.stock and not w.rep_trainable and self._ls_y is not None) else None
        self._train_policy(w.obs_b, w.state_b, w.bn_actions[:, b], w.bn_mu_probs[:, b, :self.d_action_summed_size], ls=ls_b)

    def _auto_alpha(self) -> bool:
        return bool(self.use_auto_alpha and ((self.d_action_sizes and not self.discrete_dqn_like) or self.c_action_size))

    def _same_states(self, w) -> bool:
        """the target representation's states ARE the online ones (parameter-free representation, no burn-in)"""
        return (self.burn_in_step == 0 and w.bnx_target_states.data_ptr() == w.bnx_states.data_ptr()
                and w.bnx_target_states.stride() == w.bnx_states.stride())

    def _step_after_policy_one_launch(self, w, post) -> bool:
        """One forward of the UPDATED stock policy over the whole window serves the new mu-probabilities (rows < L - 1),
        the temperature step (row b) and, where the target representation is the online one, the TD-error target
        (rows >= b): policy -> [pi(stored actions) = the new mu, the TD target's sample, the temperature step's sample] ->
        target critics on the TD sample, with the TD error's online Q of (s_b, a_b) riding along and the mu-probability
        write-back electing beside it — ONE launch (bit-identical to the chain `_step_after_policy_chain` issues).  The
        write-back's second pass rides in the TD error's return launch; the temperature step (it needs every tile's
        sample) rides in the priority update, the step's last launch, and the TD error's return, which must already see
        the new temperature, evaluates the value that step will write (`pending_alpha`).  -> False: not applicable."""
        rb, b, n = self.replay_buffer, self.burn_in_step, self.n_step
        if not (self._fused_td_chain and self.use_priority and self._same_states(w) and self._use_sidecars
                and not self._wide_critics and rb.sharded is None and self.curiosity is None and not self.use_rnd):
            return False
        B_, L_, A = *w.bnx_states.shape[:2], self.c_action_size
        f32 = dict(dtype=torch.float32, device=self.device)
        auto_alpha = self._auto_alpha()
        rows_win = StockMLP._rows(w.bnx_states, self.state_size)
        job_pi, ls_out = self._fpi.job(rows_win, None)
        probs_win = torch.empty((B_, L_, A), **f32)
        td_sample = (torch.empty((B_, L_, A), **f32), torch.empty((B_, L_), **f32))
        job_tq, td_q_table = self._ftq.job(rows_win, td_sample[0].view(-1, A))
        alpha_logp = scratch = None
        if auto_alpha:
            alpha_logp, scratch = torch.empty(B_, **f32), torch.empty((B_, A), **f32)
        job = native.pi_q_job(job_pi, job_tq, self._eps_td, td_sample[0], td_sample[1], L_,
                              action=w.bnx_actions, prob_out=probs_win,
                              eps2=self._eps_alpha if auto_alpha else None, t2=b,
                              a2_out=scratch, logp2_out=alpha_logp)
        if not native.policy_sample_q_forward_ok(job):
            return False
        if auto_alpha:
            self.noise.normal_(self._eps_alpha)
        self.noise.normal_(self._eps_td)
        xb = StockMLP._rows(w.bnx_states[:, b], self.state_size)
        ab = StockMLP._rows(w.bnx_actions[:, b], self.c_action_size)
        job_q, _ = self._fq.job(xb, ab, out=self._cq_td_buf)
        # launches off the step's critical path ride as sidecar workgroups of launches that are on it (csrc/asac_sidecar.h)
        sc_elect, post.sc_write = rb.window_scatter_sidecars(w.ids, -b, b + n, w.bnx_pad, 'mu_prob', probs_win[:, :-1])
        if auto_alpha:
            post.sc_alpha = self._alpha_sidecar(alpha_logp)
        native.policy_sample_q_forward(job, [job_q], sidecars=[sc_elect])
        if post.sc_alpha is not None:
            self._alpha_logp_over_ranks(alpha_logp)
        post.td_alpha = post.sc_alpha      # (None: a wider optimizer -> `_train_alpha`)
        post.ls_win = ls_out[0].view(B_, L_, 2 * A)
        post.probs_win, post.td_sample, post.alpha_logp = probs_win, td_sample, alpha_logp
        post.td_q_table = td_q_table.view(self.ensemble_q_num, B_, L_)
        post.side_cq = self._cq_td_buf.view(self.ensemble_q_num, -1)
        post.td_riders = [post.sc_write]
        post.mu_written = True
        return True

    def _step_after_policy_chain(self, w, post) -> None:
        """The chain form: policy forward over the window (the TD target's policy forward over the TARGET states, where
        they are not the online ones, beside it) -> ONE elementwise launch [temperature sample, pi(stored actions), TD
        target's sample] -> the TD error's online Q of (s_b, a_b) with its target ensemble on the sampled window actions
        (two networks, one launch; hosts the write-back's second pass and the temperature step as sidecars)."""
        rb, b, n = self.replay_buffer, self.burn_in_step, self.n_step
        B_, L_, A = *w.bnx_states.shape[:2], self.c_action_size
        f32 = dict(dtype=torch.float32, device=self.device)
        auto_alpha, same_states = self._auto_alpha(), self._same_states(w)
        rows_win = StockMLP._rows(w.bnx_states, self.state_size)
        td_own = self.use_priority and not same_states
        td_rows = sc_elect = None
        probs_win = torch.empty((B_, L_, A), **f32)
        # (with priorities the TD error's online-Q launch follows and hosts the second pass + the temperature step)
        if self.use_priority and self._use_sidecars and rb.sharded is None:
            sc_elect, post.sc_write = rb.window_scatter_sidecars(w.ids, -b, b + n, w.bnx_pad, 'mu_prob', probs_win[:, :-1])
        # the policy forward(s) WITH the elementwise work on their outputs as the forward launch's epilogue
        # (`native.mlp_forward_multi_sampled`: temperature sample at position b, pi(stored actions), the TD target's sample);
        # the chain form below is what it replaces, bit for bit
        if auto_alpha:
            post.alpha_logp, scratch = torch.empty(B_, **f32), torch.empty((B_, A), **f32)
        if self.use_priority and same_states:
            post.td_sample = (torch.empty((B_, L_, A), **f32), torch.empty((B_, L_), **f32))
        elif td_own:
            post.td_sample = (torch.empty((B_, n + 1, A), **f32), torch.empty((B_, n + 1), **f32))
            post.td_pi = torch.empty((B_, n + 1, A), **f32)
        job_win, ls_out = self._fpi.job(rows_win, None)
        jobs = [job_win]
        epis = None
        if native.SAMPLE_EPILOGUE and 2 * A <= 16 and w.bnx_actions.stride(-1) == 1:
            epis = [native.sample_epilogue(job_win, *((self._eps_td, *post.td_sample) if self.use_priority and same_states
                                                      else (None, None, None)), L_,
                                           action=w.bnx_actions, prob_out=probs_win,
                                           eps2=self._eps_alpha if auto_alpha else None, t2=b,
                                           a2_out=scratch if auto_alpha else None,
                                           logp2_out=post.alpha_logp if auto_alpha else None)]
        if td_own:
            td_rows = StockMLP._rows_in_place(w.nx_target_states, self.state_size)
            job_pi_td, ls_td_out = self._fpi.job(td_rows, None)
            jobs.append(job_pi_td)
            post.ls_td = ls_td_out[0].view(B_, n + 1, 2 * A)
            if epis is not None:
                epis.append(native.sample_epilogue(job_pi_td, self._eps_td, *post.td_sample, n + 1,
                                                   action=w.bnx_actions[:, b:], prob_out=post.td_pi))
        ls_win = ls_out[0].view(B_, L_, 2 * A)
        if epis is not None and not native.mlp_forward_multi_sampled_ok(jobs, epis):
            epis = None
        if auto_alpha:
            self.noise.normal_(self._eps_alpha)
        if self.use_priority:
            self.noise.normal_(self._eps_td)
        if auto_alpha and self.use_priority and self._use_sidecars and rb.sharded is None:
            post.sc_alpha = self._alpha_sidecar(post.alpha_logp)
        if epis is not None:
            native.mlp_forward_multi_sampled(jobs, epis, sidecars=[sc_elect] if sc_elect is not None else None)
        else:
            native.mlp_forward_multi(jobs)
            sq = [native.squash_job(ls_win[..., :A], ls_win[..., A:], action=w.bnx_actions, prob_out=probs_win)]
            if auto_alpha:
                sq.append(native.squash_job(ls_win[:, b, :A], ls_win[:, b, A:], self._eps_alpha, scratch, post.alpha_logp))
            if self.use_priority and same_states:
                sq.append(native.squash_job(ls_win[..., :A], ls_win[..., A:], self._eps_td, *post.td_sample))
            elif td_own:
                sq.append(native.squash_job(post.ls_td[..., :A], post.ls_td[..., A:], self._eps_td, *post.td_sample,
                                            action=w.bnx_actions[:, b:], prob_out=post.td_pi))
            native.squash_multi(sq, sidecars=[sc_elect] if sc_elect is not None else None)
        if post.sc_alpha is not None:
            self._alpha_logp_over_ranks(post.alpha_logp)
        post.ls_win, post.probs_win = ls_win, probs_win
        if self.use_priority:
            xb = StockMLP._rows(w.bnx_states[:, b], self.state_size)
            ab = StockMLP._rows(w.bnx_actions[:, b], self.c_action_size)
            riders = [sc for sc in (post.sc_write, post.sc_alpha) if sc is not None]
            if riders and self._wide_critics:
                # no critic launch to ride in: the write-back's second pass goes with the TD error's return, the temperature
                # step with the priority update (the return evaluates the value that step will write)
                post.td_riders = [post.sc_write] if post.sc_write is not None else None
                post.td_alpha = post.sc_alpha
                riders = []
            if post.td_sample is not None:
                job_q, _ = self._fq.job(xb, ab, out=self._cq_td_buf)
                job_tq, td_q_table = self._ftq.job(
                    td_rows if td_rows is not None else StockMLP._rows(w.bnx_target_states, self.state_size),
                    StockMLP._rows(post.td_sample[0], self.c_action_size))
                native.mlp_forward_multi([job_q, job_tq], sidecars=riders or None)
                post.td_q_table = td_q_table.view(self.ensemble_q_num, *post.td_sample[1].shape)
            elif riders:
                job_q, _ = self._fq.job(xb, ab, out=self._cq_td_buf)
                native.mlp_forward_multi([job_q], sidecars=riders)
            else:
                self._fq._launch_forward(xb, ab, out=self._cq_td_buf)
            post.side_cq = self._cq_td_buf.view(self.ensemble_q_num, -1)
        if post.sc_write is None:
            rb.update_window_transitions(w.ids, -b, b + n, w.bnx_pad, 'mu_prob', probs_win[:, :-1])
        post.mu_written = True

    def _step_temperature_and_aux(self, w, post) -> None:
        b = self.burn_in_step
        if self._auto_alpha() and post.sc_alpha is None:      # (a sidecar: done by the launch that carries it)
            self._train_alpha(w.obs_b, w.state_b, ls=None if post.ls_win is None else post.ls_win[:, b], logp=post.alpha_logp)
        if self.curiosity is not None:
            self._train_curiosity(w.bn_pad[:, b:], w.bnx_states[:, b:], w.bn_actions[:, b:])
        if self.use_rnd:
            self._train_rnd(w.bn_pad[:, b:], w.bnx_states[:, b:-1], w.bn_actions[:, b:])

    def _step_write_backs(self, w, post) -> None:
        """reference 2558-2605: TD error -> priorities; new behaviour probabilities and hidden states -> the ring"""
        rb, b, n, ids = self.replay_buffer, self.burn_in_step, self.n_step, w.ids
        bn_states = w.bnx_states[:, :-1]
        pi_probs = None
        if self.use_n_step_is:
            if post.probs_win is not None:
                pi_probs = post.probs_win[:, :-1]          # the last row's probability is not stored (1159-1189)
            else:
                pi_probs = self.get_l_probs([o[:, :-1] for o in w.bnx_obses_list], bn_states, w.bn_actions)
        # the hidden-state write-back rides along too: its election beside the TD error's return, its write pass beside the
        # priority update (the step's last two launches; its own election scratch: the mu-probability write pass may
        # share the return launch)
        hidden_write = None
        td_riders = list(post.td_riders or ())
        if (self.seq_hidden_state_shape[-1] != 0 and self.use_priority and self._use_sidecars
                and rb.sharded is None and bool(self.c_action_size) and not self.d_action_sizes
                and len(td_riders) < native.MAX_SIDECARS):
            hidden_rows = w.next_hidden.detach().contiguous()
            h_elect, hidden_write = rb.window_scatter_sidecars(ids, 1 - b, b + n, w.bnx_pad, 'pre_seq_hidden_state',
                                                               hidden_rows, side=True)
            td_riders.append(h_elect)
        if self.use_priority:
            # no write pass waiting for the update's launch: the TD error's return and the priority update are one launch
            # (one workgroup forms every return: it pays while each of its threads has at most one step of one window —
            # measured: B 256 n 4 +2.5 %, B 512 n 3 -0.8 %, B 1024 n 3 -0.3 %)
            merged = (self._fused_td_update and hidden_write is None and self._use_sidecars
                      and bool(self.c_action_size) and not self.d_action_sizes and ids.numel() * n <= 1024
                      and rb.td_update_ok(ids, n))
            own_td_policy = post.td_pi is not None     # the TD target's policy ran over the target states
            td, updated = self._get_td_error(
                w.bn_last[:, b:], w.bn_pad[:, b:], w.nx_obs, bn_states[:, b], w.nx_target_states, w.bnx_actions[:, b:],
                w.bn_rewards[:, b:], w.bn_dones[:, b:], pi_probs[:, b:] if self.use_n_step_is else None,
                ls=None if post.td_sample is None else (post.ls_td if own_td_policy else post.ls_win),
                sample=post.td_sample,
                stored_pi=None if post.td_sample is None else (post.td_pi if own_td_policy else post.probs_win),
                c_q=post.side_cq, q_table=post.td_q_table,
                sidecars=td_riders or None, pending_alpha=post.td_alpha, td_update=(rb, ids) if merged else None)
            if not updated:     # (else the return's launch ran the temperature step and the update)
                rb.update(ids, td, sidecars=[sc for sc in (post.td_alpha, hidden_write) if sc is not None] or None)
        if self.seq_hidden_state_shape[-1] != 0 and hidden_write is None:
            rb.update_window_transitions(ids, 1 - b, b + n, w.bnx_pad, 'pre_seq_hidden_state',
                                         w.next_hidden.detach().contiguous())
        if self.use_n_step_is and not post.mu_written:
            rb.update_window_transitions(ids, -b, b + n, w.bnx_pad, 'mu_prob', pi_probs)

    def _try_capture(self) -> None:
        """Warm up on a side stream, then capture `_device_step` into one hipGraph."""
        if not CapturedStep.api_ok():
            self._graph_failed = True
            self._logger.warning('this torch build has no CUDAGraph(keep_graph=True) / raw_cuda_graph() / instantiate(): captured '
                                 'memset nodes could not be repaired (they take effect on the first replay only on this '
                                 'ROCm), so the train step is NOT captured and runs eagerly — several times slower')
            return
        try:
            self._graph = CapturedStep.capture(self._device_step, self.device, logger=self._logger)
            self._graph_memsets = self._graph.memsets
            # (logp, scale) of the policy step live in THIS graph's private pool: whichever graph ran last is the one
            # whose tensors `_refresh_policy_stats` must read (a k-step run has its own, `train_steps`)
            self._graph.payload = self._pi_stats_src
            self._logger.info('train step captured into a hipGraph')
        except Exception as e:   # user models with host syncs etc.: stay eager, loudly
            self._graph_failed = True
            self._graph = None
            torch.cuda.synchronize()
            self._logger.warning(f'hipGraph capture of the train step failed, staying eager: {e!r}')

    def _replay_graph(self) -> None:
        self._pi_stats_src = self._graph.payload
        self._graph.replay(self._direct_graph_launch, self._logger)

    def _ready_to_train(self) -> bool:
        """Reference `train` 2503-2506: no step until the buffer holds more than a batch.  A data-parallel step holds
        collectives, so the ranks decide TOGETHER (one small all-reduce per call until it turns true, none afterwards):
        throughput mode needs every rank's shard above its own batch; parity mode needs the UNION above the global batch
        (and every rank to know the transition layout: it allocates its batch from it) — a rank with a short shard
        takes part from the first step."""
        if not self.use_replay_buffer:
            return self.batch_buffer.has_batch      # (the host mirror of the queue: no synchronisation)
        rb = self.replay_buffer
        if self._dist is None:
            return rb.is_lg_batch_size
        if self._dist_ready:
            return True
        if rb.sharded is not None:
            all_have_keys, union = self._dist.all_ready(rb._columns is not None and bool(rb._columns), rb.size, self.device)
            self._dist_ready = all_have_keys and union > rb.sharded.B
        else:
            self._dist_ready, _ = self._dist.all_ready(rb.is_lg_batch_size, rb.size, self.device)
        return self._dist_ready

    def _optimizer_hp(self) -> tuple:
        """(lr, betas, eps) of every optimizer of the learner: host floats that a captured step holds as kernel arguments"""
        opts = self._all_optimizers
        if opts is None:      # (collected once: `train()` is the host's hot loop)
            opts = self._all_optimizers = [o for o in vars(self).values() if isinstance(o, FlatAdam)] + \
                [o for o in self.optimizer_q_list if o is not None]
        return tuple((o.lr, o.betas, o.eps) for o in opts)

    def _drop_graphs(self) -> None:
        """every captured graph of the learner: the step's, the lookahead's per parity, the k-step runs'"""
        self._graph, self._la_graphs, self._graph_runs = None, {}, {}

    def _drop_graphs_if_hp_changed(self) -> None:
        """a learning rate (betas, eps) changed after capture — a schedule, a user edit — would otherwise go unnoticed by
        every replay: the graphs are dropped and the step is captured again with the new values"""
        hp = self._optimizer_hp()
        if hp != self._graph_hp:
            if self._graph_hp is not None and (self._graph is not None or self._la_graphs or self._graph_runs):
                self._logger.info('optimizer hyper-parameters changed: the captured step is dropped and captured again')
                self._drop_graphs()
            self._graph_hp = hp

    @unified_elapsed_timer('train a step', 10)
    def train(self) -> int:
        step = self.get_global_step()
        rb = getattr(self, 'replay_buffer', None)
        if not self._ready_to_train():
            self._profiler('train a step').ignore()
            return step
        self._drop_graphs_if_hp_changed()
        if rb is None:
            if self.batch_buffer._batch is None:
                self.batch_buffer.build_static()
                self._drop_graphs()
        elif rb._gather_keys is None:
            rb._build_batch()
            self._drop_graphs()
        if rb is not None:
            self._head_gather_plan(rb, build=True)      # (host work, once per static set: before any capture)

        if self._lookahead:
            if not rb.lookahead:
                rb.enable_lookahead()
            if not rb.next_valid:
                # the very first batch (the reference's thread has drawn two before the first `sample()` returns)
                with torch.cuda.device(self.device):
                    rb.sample_next_into_static()
            rb.swap_sets()
            # the captured step holds the sets' addresses: one graph per arrangement, taken in turn
            self._graph = self._la_graphs.get(rb.parity)
            rb.next_valid = False

        with self._profiler('train', repeat=10):
            if self.update_target_per_step != 1 and step % self.update_target_per_step == 0:
                self._update_target_variables(tau=self.tau)
            graph_ok = (self._use_graph and not self._graph_failed and isinstance(self.noise, DeviceNoise)
                        and (self._dist is None or self._graph_collectives))
            if graph_ok and self._graph is None and self._eager_steps >= self._graph_warmup:
                self._try_capture()
            if graph_ok and self._graph is not None:
                self._replay_graph()
            else:
                self._device_step()
                self._eager_steps += 1
        if rb is None:
            self.batch_buffer.pop_host()
        if self._lookahead:
            self._la_graphs[rb.parity] = self._graph
            rb.next_valid = True

        # host synchronisation points the reference has too: here the NaN flag of the priority update kernels is
        # read back, so a diverged run raises the reference's 'td_error has nan' (replay_buffer.py:418-420) within
        # `write_summary_per_step` steps instead of training on with frozen priorities
        if step % self.write_summary_per_step == 0:
            if rb is not None:
                rb.check_health()
            if self.summary_writer is not None:
                self._write_train_summaries(step)
        if step % self.save_model_per_step == 0:
            self.save_model()
        return self.increase_global_step()

    def train_steps(self, n_steps: int) -> int:
        """`n_steps` consecutive `train()` calls.  Where the step already replays as a hipGraph and nothing has to
        happen on the host between the steps of this run (target update every step, no summary / health check / checkpoint
        falling due inside it), the run is ONE replay of a graph holding `n_steps` steps: the boundary between two graph
        launches costs ~4.6 us more than a kernel boundary inside one (cfg2: 92.9 us per step as one step per launch,
        89.7 as two, 88.3 as four).  Same launches, same order, same device-side counters and draws: the state after the
        run is that of the `train()` calls bit for bit.  Episodes enter between runs, not between the steps of one."""
        k = int(n_steps)
        step = self.get_global_step()
        rb = getattr(self, 'replay_buffer', None)
        self._drop_graphs_if_hp_changed()
        due = any((step + i) % self.write_summary_per_step == 0 or (step + i) % self.save_model_per_step == 0
                  for i in range(k))
        # (batch mode: each step of the run pops a batch — at least k must be queued)
        data_ok = (len(self.batch_buffer) >= k and self.batch_buffer._batch is not None) if rb is None else \
            (rb.is_lg_batch_size and rb._gather_keys is not None)
        if (k <= 1 or due or self._lookahead or self._graph is None or self._graph.exec_handle is None
                or self.update_target_per_step != 1 or not data_ok):
            for _ in range(k):
                step = self.train()
            return step
        cached = self._graph_runs.get(k)
        if cached is None or cached.beside is not self._graph:      # (captured per run length; dropped with the step's graph)
            def k_steps():
                for _ in range(k):
                    self._device_step()
            try:
                run = CapturedStep.capture(k_steps, self.device, take_exec=True, logger=self._logger)
                self._graph_memsets = run.memsets
                run.payload = self._pi_stats_src      # the run's last step leaves its (logp, scale) in the run graph's pool
            except Exception as e:
                run = None
                torch.cuda.synchronize()
                self._logger.warning(f'hipGraph capture of a {k}-step run failed, replaying single steps: {e!r}')
            cached = self._graph_runs[k] = _GraphRun(self._graph, run)
        if cached.run is None:
            for _ in range(k):
                step = self.train()
            return step
        self._pi_stats_src = cached.run.payload
        with self._profiler('train', repeat=10):
            cached.run.replay()
        if rb is None:
            for _ in range(k):
                self.batch_buffer.pop_host()
        self.global_step.add_(k)
        return self.global_step.item()

    @torch.no_grad()
    def _refresh_policy_stats(self, log_c_alpha: torch.Tensor | None = None) -> None:
        """The stock policy step forms its gradients on chip and leaves the logged statistics (policy
        objective, Gaussian entropy) to be computed here, on demand, from the step's buffers.  The objective
        is weighted by the temperature: by default the current one (already moved by the step's temperature
        update, which is what a log line sees); `log_c_alpha` = the value the policy step itself used."""
        if self._pi_stats_src is None:
            return
        logp, scale, *off = self._pi_stats_src
        E, Es = self.ensemble_q_num, self.ensemble_q_sample
        native.policy_loss_fwd_bwd(logp, self._pi_q.view(E, -1), self._subsets['pi_c'] if Es != E else None, Es,
                                   self.log_c_alpha if log_c_alpha is None else log_c_alpha, scale,
                                   self._stats['loss_policy'],
                                   torch.empty_like(self._grad_logp), torch.empty_like(self._grad_q),
                                   self._stats['c_entropy'])
        if off:     # the offline loss' term of the step: (loc | scale) rows, noise, stored actions
            native.policy_offline_term(off[0], off[1], off[2], self._stats['loss_policy'])

    def _write_train_summaries(self, step: int) -> None:
        self.summary_available = True
        self._refresh_policy_stats()
        w = self.summary_writer
        if self.use_replay_buffer:
            w.add_scalar('metric/replay_id', self.replay_buffer.get_curr_id(), step)
        w.add_scalar('loss/q', self._stats['loss_q'].item(), step)
        if self.d_action_sizes:
            w.add_scalar('loss/d_entropy', self._stats['d_entropy'].item(), step)
            if self.use_auto_alpha:
                w.add_scalar('loss/d_alpha', torch.exp(self.log_d_alpha).item(), step)
        if self.c_action_size:
            w.add_scalar('loss/c_entropy', self._stats['c_entropy'].item(), step)
            if self.use_auto_alpha:
                w.add_scalar('loss/c_alpha', torch.exp(self.log_c_alpha).item(), step)
        if self.curiosity is not None:
            w.add_scalar('loss/curiosity', self._stats['loss_curiosity'].item(), step)
        w.flush()

    def close(self):
        self._closed = True
        # captured graphs go first (they hold the collectives' kernels of a data-parallel step: a process group must
        # not be torn down under them)
        self._drop_graphs()
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        if hasattr(self, 'replay_buffer'):
            self.replay_buffer.close()


def nn_parameter_scalar(value: float, device) -> torch.nn.Parameter:
    return torch.nn.Parameter(torch.tensor(value, dtype=torch.float32, device=device), requires_grad=True)
