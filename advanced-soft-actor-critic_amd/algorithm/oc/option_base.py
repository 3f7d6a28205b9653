"""`OptionBase` — the learner of ONE option of the option-critic, the drop-in for the reference's
`algorithm/oc/option_base.OptionBase` (`option_base.py:12-801`): a `SAC_Base` without a replay buffer and without a
sampling thread, plus a termination head.  The option selector drives it with tensors it has already sampled and
encoded; `train()` is not an entry point of this class.

What runs where:
  * `_get_y`, continuous branch: policy over the window, rsample / tanh / log-prob and pi(stored actions) in one launch
    (`asac_squash_sample_fwd`: the parent's `_window_sample`), the target critics, the return's arguments assembled by
    the parent's `_c_return`, then ONE launch for subset minimum, termination mix, mean over the
    options, ratios and the V-trace scan (`asac_option_return`, csrc/option.hip); with the online critics' values handed
    in (`_get_td_error`, continuous-only action spaces) the same launch writes mean_e |q_e - y|.
  * `_get_y`, discrete branches alone with a policy (`fused_option_discrete_applies`, `hip_config['fused_option_discrete']`):
    the policy's logits and the target critics' head outputs over the window, then ONE launch for the subset minimum per
    action entry, branch softmax, the termination mix with the mean over the options, ratios and the V-trace scan
    (`asac_option_discrete_return`, csrc/discrete.hip); `_get_td_error` hands the online heads at t = 0 to the same launch
    and takes mean_e |q_e - y| from it; `compute_rep_q_grads` forms the Q loss and its gradient at the heads with
    `asac_discrete_q_loss_grad` and back-propagates from there.  Hybrid and DQN-like options, sizes over the launches'
    limits and the switch off run torch compositions that end in `asac_vtrace_return_direct` / `get_dqn_like_d_y`, as
    the parent's.
  * `compute_rep_q_grads` leaves gradients in the flat gradient buffer (clipped double-Q loss and d loss / d q from
    `asac_q_loss_fwd_bwd` for continuous-only action spaces), `train_rep_q` applies Adam to the [rep | q_0 .. q_E-1] span in
    one launch (`asac_adam_step`).  `train_policy_alpha` is the parent's `_train_policy`, `_train_alpha`, `_train_curiosity`,
    `_train_rnd`, unchanged.
  * `compute_termination_grads`: the head's forward, then value and d loss / d beta from ONE launch
    (`asac_termination_loss_grad`), then the head's backward; `train_termination` applies Adam to the head's span, with
    moments and a step count of its own (`imitation_base.SpanAdam`, saved in `torch.optim.Adam`'s format).
  * `_update_target_variables`: the parent's Polyak launch plus one more `asac_polyak` over the termination head's flat
    target buffer.
The three groups of optimizers (representation + critics; policy, temperatures, curiosity, RND; termination) keep a step
count each, advanced by their `train_*` call: the selector may call them at different rates, as the reference's
per-optimizer counts allow.

Not supported, rejected at construction: `siamese`, `use_prediction`, a data-parallel context (`hip_config['dist']`),
`SEQ_ENCODER.ATTN` (the reference raises for it in `get_l_states`).  The training calls take batches of exactly
`batch_size` rows (`_check_batch`).  An option's calls are not captured into a hipGraph:
the selector owns the step, capture belongs with it.
Differences from the reference, both inherited from the parent's fused pieces: pi(stored actions) clamps the stored action
to +-0.999 before atanh (`asac_squash_sample_fwd`, as `SAC_Base._get_y` and acting do; option_base.py:415 does not, and
gives inf / NaN for a stored action of exactly +-1), and infinite per-dimension probabilities count as 1 in the products.
"""
import inspect
import logging
import os

import torch
from torch.nn import functional

from asac_amd import native

from ..fused import FlatParamGroup
from ..imitation_base import SpanAdam
from ..param_grads import learner_backward
from ..sac_base import SAC_Base
from ..utils.enums import SEQ_ENCODER
from ..utils.operators import get_last_false_indexes

_UNSUPPORTED = "OptionBase does not support {what}: {why}"


def _reject_unsupported(args, kwargs) -> None:
    """the constructor arguments this class cannot honour, looked at before anything touches a device"""
    bound = inspect.signature(SAC_Base.__init__).bind_partial(None, *args, **kwargs).arguments
    if bound.get('siamese') is not None:
        raise ValueError(_UNSUPPORTED.format(
            what='siamese', why='the siamese representation loss inside compute_rep_q_grads is not built for an option'))
    if bound.get('use_prediction'):
        raise ValueError(_UNSUPPORTED.format(
            what='use_prediction', why='the prediction models inside compute_rep_q_grads are not built for an option'))
    if (bound.get('hip_config') or {}).get('dist') is not None:
        raise ValueError(_UNSUPPORTED.format(
            what="a data-parallel context (hip_config['dist'])", why='an option is a single-GPU learner'))
    if bound.get('seq_encoder') == SEQ_ENCODER.ATTN:
        raise ValueError(_UNSUPPORTED.format(
            what='SEQ_ENCODER.ATTN', why='seq_encoder in option cannot be ATTN (option_base.py:180-181)'))


def fused_option_discrete_applies(*, enabled, d_action_sizes, c_action_size, discrete_dqn_like, float32_on_device,
                                  ensemble_q_num, n_step, batch_size, num_options) -> bool:
    """Do the return, the TD error and the Q loss of an option of this configuration run on `asac_option_discrete_return`
    / `asac_discrete_q_loss_grad` (`hip_config['fused_option_discrete']`)?  Only with discrete branches alone and a policy
    (no DQN-like target), on float32 device tensors, within the entry points' size limits, `batch_size` rows a batch
    and `num_options` options' values a step.  Everything else runs the eager code."""
    return bool(enabled and len(d_action_sizes) > 0 and c_action_size == 0 and not discrete_dqn_like and float32_on_device
                and native.discrete_sizes_ok(d_action_sizes, ensemble_q_num, n_step, batch_size)
                and 0 < num_options <= native.OPTION_MAX_OPTIONS)


class OptionBase(SAC_Base):
    _plain_learner = False

    def __init__(self, option: int, display_name: str, fix_policy: bool, random_q: bool, *args, **kwargs):
        self.option = option
        self.display_name = display_name
        self.fix_policy = fix_policy
        if os.environ.get('DISABLE_RANDOM_Q') is not None:
            random_q = False
        self.random_q = random_q
        _reject_unsupported(args, kwargs)
        super().__init__(*args, **kwargs)
        # the parent's one-launch discrete path is the plain learner's (the option's own `_get_y` / `_get_td_error` mix
        # the termination in and take the minimum over the critics): off; the option's own launch has its own switch
        self._fused_discrete = False
        self._fused_dqn = False         # (its own `get_dqn_like_d_y` mixes the termination in as well)
        hip_config = inspect.signature(SAC_Base.__init__).bind_partial(None, *args, **kwargs).arguments.get('hip_config')
        self._fused_option_discrete = bool((hip_config or {}).get('fused_option_discrete', True))

    # -- construction (option_base.py:27-86) ----------------------------------------------------------------------------
    def _sample_thread(self):
        pass

    def _set_logger(self):
        self._logger = logging.getLogger('option' if self.ma_name is None else f'option.{self.ma_name}')

    def _init_replay_buffer(self, replay_config=None) -> None:
        # no replay buffer, no episode queue, no prefetch: the selector owns the data.  The flag guards the parent's own
        # buffer accesses (restore, save)
        self.use_replay_buffer = False

    def train(self):
        raise RuntimeError('OptionBase.train is not an entry point: the option selector drives compute_rep_q_grads / '
                           'train_rep_q / train_policy_alpha / compute_termination_grads / train_termination')

    def train_steps(self, n_steps: int):
        return self.train()

    def put_episode(self, *args, **kwargs) -> None:
        raise RuntimeError('OptionBase holds no replay buffer: episodes go to the option selector')

    def _build_aux(self, nn_mod, test_obs_list) -> list:
        """the termination head joins the learner's flat parameter buffer as the segment `termination` (behind the parent's
        optional heads); its target copy gets a flat buffer of its own for the Polyak launch"""
        named = super()._build_aux(nn_mod, test_obs_list)
        dev = self.device
        self.model_termination = nn_mod.ModelTermination(self.state_size).to(dev)
        self.model_target_termination = nn_mod.ModelTermination(self.state_size).to(dev)
        for p in self.model_target_termination.parameters():
            p.requires_grad = False
        if self.fix_policy:     # option_base.py:43-47 (before the flat buffer binds the gradients: these get none)
            for p in self.model_rep.parameters():
                p.requires_grad = False
            for p in self.model_policy.parameters():
                p.requires_grad = False
        named.append(('termination', list(self.model_termination.parameters())))
        return named

    def _build_model(self, nn, nn_config, init_log_alpha, learning_rate) -> None:
        super()._build_model(nn, nn_config, init_log_alpha, learning_rate)
        dev = self.device
        self._target_termination_params = FlatParamGroup(
            [('termination', list(self.model_target_termination.parameters()))], dev, with_grad=False)
        self.optimizer_termination = SpanAdam(self._params, ['termination'], learning_rate)
        # a step count per group of optimizers (the parent's learner has one, advanced once per `train`)
        self._steps_rep_q = self._opt_steps
        self._steps_pi = torch.zeros(1, dtype=torch.int64, device=dev)
        for name in ('optimizer_policy', 'optimizer_alpha', 'optimizer_curiosity', 'optimizer_rnd'):
            opt = getattr(self, name, None)
            if opt is not None:
                opt.steps_done = self._steps_pi
        f32 = dict(dtype=torch.float32, device=dev)
        self._loss_termination = torch.zeros(1, **f32)
        self._stats['loss_termination'] = self._loss_termination[0]
        self._stats['termination'] = torch.zeros((), **f32)
        # exchange words of the termination loss launch, this learner's own: a selector's options may run on different
        # streams, and a workspace serves one launch at a time
        self._termination_ws = torch.zeros(int(native.load().asac_termination_loss_grad_workspace()), **f32)

    def _build_ckpt(self) -> None:
        super()._build_ckpt()
        self.ckpt_dict['model_termination'] = self.model_termination
        self.ckpt_dict['model_target_termination'] = self.model_target_termination

    def _init_or_restore(self, last_ckpt) -> None:
        super()._init_or_restore(last_ckpt)
        self._target_termination_params.rebind()
        if self.train_mode and self.random_q:
            # fresh critics for this option (option_base.py:64-72): matrices He-normal, vectors standard normal, written
            # in place so that the parameters stay views of the flat buffer; the targets then take them over (tau = 1)
            with torch.no_grad():
                for p in (p for q in self.model_q_list for p in q.parameters()):
                    (torch.nn.init.kaiming_normal_ if p.dim() > 1 else torch.nn.init.normal_)(p)
            self._logger.warning('Model Q randomized')
            self._update_target_variables()

    def remove_models(self, gt: int):
        """drop every checkpoint of this option that is newer than step `gt` (option_base.py:74-86)"""
        newer = [] if self.ckpt_dir is None else [f for f in self.ckpt_dir.glob('*.pth') if int(f.stem) > gt]
        for path in newer:
            try:
                path.unlink()
            except OSError as e:
                self._logger.error(f'Failed to delete {path}: {e}')
            else:
                self._logger.warning(f'{path.name} deleted')

    @torch.no_grad()
    def _update_target_variables(self, tau=1.) -> None:
        """option_base.py:88-98: the termination head's Polyak update is one more launch over its flat buffers"""
        tp = self._target_termination_params
        s, e = self._params.span('termination')
        if e > s:
            native.polyak(tp.flat[:e - s], self._params.flat[s:e], tau)
        return super()._update_target_variables(tau)

    # -- acting (option_base.py:100-144) -----------------------------------------------------------------------------
    @torch.no_grad()
    def choose_action(self, obs_list, pre_action, pre_seq_hidden_state, offline_action=None, disable_sample=False,
                      force_rnd_if_available=False):
        """device tensors in, device tensors out, as the reference's: -> (action [batch, action_size], prob [batch,
        action_size], seq_hidden_state [batch, *seq_hidden_state_shape], termination [batch])"""
        obs_list = list(obs_list)
        state, seq_hidden_state = self.model_rep([o.unsqueeze(1) for o in obs_list], pre_action.unsqueeze(1),
                                                 pre_seq_hidden_state.unsqueeze(1))
        state, seq_hidden_state = state.squeeze(1), seq_hidden_state.squeeze(1)
        action, prob = self._choose_action(obs_list, state, offline_action, disable_sample or self.fix_policy,
                                           force_rnd_if_available)
        termination = self.model_termination(state, obs_list)
        return action, prob, seq_hidden_state, termination.squeeze(-1)

    # -- states (option_base.py:148-181) -----------------------------------------------------------------------------
    def get_l_states(self, l_indexes, l_padding_masks, l_obses_list, l_pre_actions, l_pre_seq_hidden_states,
                     is_target=False):
        if self.seq_encoder == SEQ_ENCODER.ATTN:
            raise Exception('seq_encoder in option cannot be ATTN')
        return super().get_l_states(l_indexes, l_padding_masks, l_obses_list, l_pre_actions, l_pre_seq_hidden_states,
                                    is_target=is_target)

    # -- targets (option_base.py:185-429) ----------------------------------------------------------------------------
    @torch.no_grad()
    def get_dqn_like_d_y(self, n_terminations, next_n_vs, n_last_masks, n_padding_masks, n_rewards, n_dones,
                         stacked_next_n_d_qs, stacked_next_target_n_d_qs):
        """Double-DQN n-step target at the last valid step of each row, with the termination mix on the bootstrap value
        (option_base.py:186-246; `sac_aux.get_dqn_like_d_y` is the parent's form without the mix) -> y [batch, 1]"""
        rows = torch.arange(n_padding_masks.shape[0], device=self.device)
        last = get_last_false_indexes(torch.logical_or(n_last_masks, n_padding_masks), dim=1)
        at_last = lambda x: x[rows, last].unsqueeze(-1)  # noqa: E731
        next_q = stacked_next_n_d_qs[:, rows, last, :]
        next_t = stacked_next_target_n_d_qs[:, rows, last, :]
        greedy = torch.cat([functional.one_hot(torch.argmax(part, dim=-1), size)
                            for part, size in zip(next_q.split(self.d_action_sizes, dim=-1), self.d_action_sizes)], dim=-1)
        picked = torch.sum(next_t * greedy, dim=-1, keepdim=True) / self.d_action_branch_size
        boot, _ = torch.min(picked, dim=0)
        beta = at_last(n_terminations)
        boot = (1 - beta) * boot + beta * at_last(next_n_vs)
        g = torch.sum(self._gamma_ratio * n_rewards, dim=-1, keepdim=True)
        return g + torch.pow(self.gamma, last.unsqueeze(-1) + 1) * boot * ~at_last(n_dones)

    def _draw_subset(self, key):
        sub = self._subsets[key]
        self.noise.subset_(sub, self.ensemble_q_num)
        return sub

    def _option_discrete_fused(self, B: int, num_options: int) -> bool:
        """this call's discrete arithmetic runs on the option's launches (`fused_option_discrete_applies`)"""
        return fused_option_discrete_applies(
            enabled=self._fused_option_discrete, d_action_sizes=self.d_action_sizes, c_action_size=self.c_action_size,
            discrete_dqn_like=self.discrete_dqn_like,
            float32_on_device=self._params.flat.dtype == torch.float32 and self._params.flat.is_cuda,
            ensemble_q_num=self.ensemble_q_num, n_step=self.n_step, batch_size=B, num_options=num_options)

    def _get_d_y_fused(self, next_n_vs_over_options, n_terminations, n_last_masks, n_padding_masks, nx_obses_list,
                       nx_states, n_actions, n_rewards, n_dones, n_mu_probs, subset_prefix, d_q_online, td_out):
        """option_base.py:287, 333-373 (and, with `d_q_online`, the TD error) as ONE launch -> d_y [batch, 1]: no
        distribution objects, no stack of the members' head outputs; the subsets are drawn in the eager branch's order"""
        B = n_rewards.shape[0]
        no_c = torch.zeros(0, device=self.device)
        logits = self._discrete_logits(nx_states, nx_obses_list)
        heads = [q(nx_states, no_c, nx_obses_list)[0] for q in self.model_target_q_list]       # [B, n+1, D] each
        sub_next, sub_n = self._draw_subset(subset_prefix + '_dnext'), self._draw_subset(subset_prefix + '_dn')
        # (a fresh tensor per call: the selector keeps the returned y for the termination step)
        d_y = torch.empty(B, dtype=torch.float32, device=self.device)
        args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, d_y)
        args.subset_n, args.subset_next, args.E_sample = sub_n.data_ptr(), sub_next.data_ptr(), self.ensemble_q_sample
        args.log_alpha = self.log_d_alpha.data_ptr()
        if self.use_n_step_is:
            if n_mu_probs.stride(-1) != 1:
                n_mu_probs = n_mu_probs.contiguous()
            args.mu_prob, args.mu_stride_b, args.mu_stride_t = n_mu_probs.data_ptr(), n_mu_probs.stride(0), n_mu_probs.stride(1)
        if d_q_online is not None:
            args.td_error_out = td_out.data_ptr()
        if n_actions.stride(-1) != 1:
            n_actions = n_actions.contiguous()
        native.option_discrete_return(args, self._branches, heads, logits, n_terminations, next_n_vs_over_options,
                                      action=n_actions, q_online=d_q_online)
        return d_y.unsqueeze(-1)

    @torch.no_grad()
    def _get_y(self, next_n_vs_over_options, n_terminations, n_last_masks, n_padding_masks, nx_obses_list, nx_states,
               n_actions, n_rewards, n_dones, n_mu_probs, *, eps_buf=None, subset_prefix='y', y_out=None, q_online=None,
               td_out=None, d_q_online=None):
        """option_base.py:249-429 -> (d_y [batch, 1] | None, c_y [batch, 1] | None).  The keyword-only arguments are
        this class's: the noise buffer and the ensemble subsets to draw into, where the continuous return goes, and the
        online critics' values [E, batch] (`d_q_online`: their discrete head outputs [batch, D] each, pure-discrete
        option on its own launch) whose TD error the return's launch forms as well."""
        B, n = n_rewards.shape
        A = self.c_action_size
        f32 = dict(dtype=torch.float32, device=self.device)
        if self._option_discrete_fused(B, next_n_vs_over_options.shape[-1]):
            n_last_masks, n_padding_masks, n_dones = (m.contiguous() for m in (n_last_masks, n_padding_masks, n_dones))
            return self._get_d_y_fused(next_n_vs_over_options, n_terminations, n_last_masks, n_padding_masks,
                                       nx_obses_list, nx_states, n_actions, n_rewards, n_dones, n_mu_probs, subset_prefix,
                                       d_q_online, td_out), None
        if y_out is None:       # (a fresh tensor per call: the selector keeps the returned y for the termination step)
            y_out = torch.empty(B, **f32)
        nx_actions = torch.cat([n_actions, torch.zeros_like(n_actions[:, :1])], dim=1)
        n_last_masks, n_padding_masks, n_dones = (m.contiguous() for m in (n_last_masks, n_padding_masks, n_dones))
        d_policy, c_policy, loc, scale, plain = self._policy(nx_states, nx_obses_list)

        logp = c_pi = None
        if A:
            if eps_buf is None or eps_buf.shape != (B, n + 1, A):
                eps_buf = torch.empty((B, n + 1, A), **f32)
            a_tanh, logp, c_pi = self._window_sample(loc, scale, plain, c_policy, eps_buf, nx_actions)
        else:
            a_tanh = torch.zeros(0, device=self.device)

        d_y = c_y = None
        nx_qs = None
        if self.d_action_sizes:
            nx_qs = [q(nx_states, a_tanh, nx_obses_list) for q in self.model_target_q_list]
            vbar = next_n_vs_over_options.mean(-1)                                          # option_base.py:287
            stacked = torch.stack([q[0] for q in nx_qs])                                   # [E, B, n+1, D]
            sub_next = self._draw_subset(subset_prefix + '_dnext')
            next_target = stacked[:, :, 1:].index_select(0, sub_next.long())
            if self.discrete_dqn_like:      # 313-332
                next_c = a_tanh[:, 1:] if A else a_tanh
                next_obs = [o[:, 1:] for o in nx_obses_list]
                eval_next = torch.stack([q(nx_states[:, 1:], next_c, next_obs)[0] for q in self.model_q_list])
                sub_eval = self._draw_subset(subset_prefix + '_dn')
                d_y = self.get_dqn_like_d_y(n_terminations, vbar, n_last_masks, n_padding_masks, n_rewards, n_dones,
                                            eval_next.index_select(0, sub_eval.long()), next_target)
            else:                           # 333-373: the MINIMUM over the sampled critics (the parent takes the mean)
                sub_n = self._draw_subset(subset_prefix + '_dn')
                min_n = stacked[:, :, :-1].index_select(0, sub_n.long()).min(0)[0]
                min_next = next_target.min(0)[0]
                probs = d_policy.probs
                n_p, next_p = probs[:, :-1], probs[:, 1:]
                d_alpha = torch.exp(self.log_d_alpha)
                beta = n_terminations.unsqueeze(-1)
                tmp_n_vs = min_n - d_alpha * torch.log(n_p.clamp(min=1e-8))
                tmp_next = (1 - beta) * (min_next - d_alpha * torch.log(next_p.clamp(min=1e-8))) + beta * vbar.unsqueeze(-1)
                v_n = torch.sum(n_p * tmp_n_vs, dim=-1) / self.d_action_branch_size
                v_next = torch.sum(next_p * tmp_next, dim=-1) / self.d_action_branch_size
                pi, mu = self._stored_action_ratios(d_policy, n_mu_probs, nx_actions) if self.use_n_step_is else (None, None)
                d_y = torch.empty(B, **f32)
                args = self._vtrace_args(n_rewards, n_dones, n_last_masks, n_padding_masks, d_y)
                native.vtrace_return_direct(args, v_n.contiguous(), v_next.contiguous(), pi, mu)
                d_y = d_y.unsqueeze(-1)

        if A:       # 375-427: one launch
            sub_n, sub_next = self._draw_subset(subset_prefix + '_cn'), self._draw_subset(subset_prefix + '_cnext')
            if nx_qs is not None:
                q_tab = torch.stack([q[1] for q in nx_qs]).squeeze(-1)                      # [E, B, n+1]
            else:
                q_tab = self._c_q_values(True, nx_states, a_tanh, nx_obses_list)
            ret = self._c_return(q_tab, logp, c_pi, n_mu_probs, sub_n, sub_next, n_rewards, n_dones, n_last_masks,
                                 n_padding_masks, y_out, q_online, td_out)
            native.option_return(ret.args, n_terminations, next_n_vs_over_options)
            c_y = y_out.unsqueeze(-1)
        return d_y, c_y

    def _target_terminations(self, nx_target_states, nx_target_obses_list):
        with torch.no_grad():
            beta = self.model_target_termination(nx_target_states[:, :-1], [o[:, :-1] for o in nx_target_obses_list])
        return beta.squeeze(-1)

    # -- representation and critics (option_base.py:431-610) ---------------------------------------------------------
    def compute_rep_q_grads(self, next_n_vs_over_options, n_indexes, n_last_masks, n_padding_masks, nx_obses_list,
                            nx_target_obses_list, nx_states, nx_target_states, n_actions, n_pre_actions, n_rewards,
                            n_dones, n_mu_probs, n_pre_seq_hidden_states, priority_is=None):
        """Leaves d loss_q / d (representation, critics) in the flat gradient buffer -> (d_y, c_y)"""
        self._check_batch(n_rewards.shape[0])
        E, dsum = self.ensemble_q_num, self.d_action_summed_size
        n_target_terminations = self._target_terminations(nx_target_states, nx_target_obses_list)
        obs_list = [o[:, 0] for o in nx_obses_list]
        state, action = nx_states[:, 0], n_actions[:, 0]
        d_action, c_action = action[..., :dsum], action[..., dsum:]
        B = state.shape[0]
        q_list = None
        if self.d_action_sizes:
            q_list = [q(state, c_action, obs_list) for q in self.model_q_list]
            c_q = torch.stack([q[1] for q in q_list]).squeeze(-1) if self.c_action_size else None
        else:
            c_q = self._c_q_values(False, state, c_action, obs_list)                         # [E, B]
        d_y, c_y = self._get_y(next_n_vs_over_options, n_target_terminations, n_last_masks, n_padding_masks,
                               nx_target_obses_list, nx_target_states.detach(), n_actions, n_rewards, n_dones,
                               n_mu_probs if self.use_n_step_is else None,
                               eps_buf=self._eps_y, subset_prefix='y')

        start, stop = self._params.span('rep', f'q_{E - 1}')
        self._params.grad[start:stop].zero_()                   # optimizer_rep / optimizer_q zero_grad (534-538)
        losses = roots = None
        if self._option_discrete_fused(B, next_n_vs_over_options.shape[-1]):
            # loss values and d (sum_e l_e) / d (head outputs) from one launch; back-propagation starts at the heads
            heads = [q[0] for q in q_list]
            grad_q, _ = self._discrete_grad_buffers(B)
            native.discrete_q_loss_grad(self._branches, [h.detach() for h in heads], d_action, d_y, priority_is,
                                        self._loss_q_e, grad_q)
            roots = (heads, list(grad_q.unbind(0)))
        elif self.d_action_sizes:
            qs = torch.stack([torch.sum(d_action * q[0], dim=-1, keepdim=True) / self.d_action_branch_size
                              for q in q_list])                                             # [E, B, 1]
            losses = functional.mse_loss(qs, d_y.expand_as(qs), reduction='none')
        if self.c_action_size:
            yv = c_y.reshape(1, -1)
            if self.clip_epsilon > 0:
                with torch.no_grad():
                    t_q = self._c_q_values(True, state.detach(), c_action, obs_list)
                if losses is None and B == self._grad_q.shape[1]:
                    # loss values and d (sum_e l_e) / d q from one launch; back-propagation starts at q
                    w = priority_is.reshape(-1).contiguous() if priority_is is not None else None
                    native.q_loss_fwd_bwd(c_q.detach().contiguous(), t_q.contiguous(), c_y.reshape(-1), w,
                                          self.clip_epsilon, self._loss_q_e, self._grad_q)
                    roots = ([c_q], [self._grad_q])
                else:
                    clipped = t_q + torch.clamp(c_q - t_q, -self.clip_epsilon, self.clip_epsilon)
                    c_loss = torch.maximum((clipped - yv) ** 2, (c_q - yv) ** 2).unsqueeze(-1)
            else:
                c_loss = functional.mse_loss(c_q, yv.expand_as(c_q), reduction='none').unsqueeze(-1)
            if roots is None:
                losses = c_loss if losses is None else losses + c_loss
        if roots is None:
            if priority_is is not None:
                losses = losses * priority_is.unsqueeze(0)
            loss_q_list = losses.mean(dim=(1, 2))
            self._loss_q_e.copy_(loss_q_list.detach())
            roots = ([loss_q_list.sum()], [None])
        with learner_backward():
            torch.autograd.backward(*roots, retain_graph=True)
        self._write_option_summary({'loss/q': self._stats['loss_q']})
        return d_y, c_y

    def train_rep_q(self):
        """optimizer_q steps, then optimizer_rep (605-610): adjacent segments, one Adam launch"""
        start, stop = self._params.span('rep', f'q_{self.ensemble_q_num - 1}')
        if self.fix_policy or self.optimizer_rep is None:
            start = self._params.span('q_0')[0]
        self.optimizer_q_list[0].step(start, stop)
        self._steps_rep_q.add_(1)

    # -- policy, temperatures, curiosity, RND (option_base.py:612-673) -----------------------------------------------
    def train_policy_alpha(self, n_padding_masks, n_obses_list, nx_states, n_actions, n_mu_probs) -> None:
        if self.fix_policy:
            return
        self._check_batch(n_actions.shape[0])
        obs_list = [o[:, 0] for o in n_obses_list]
        n_states = nx_states[:, :-1]
        state, action = n_states[:, 0], n_actions[:, 0]
        mu_d_policy_probs = n_mu_probs[:, 0, :self.d_action_summed_size]
        for name in ('policy', 'alpha', 'curiosity', 'rnd'):
            if name in self._params.segments:
                s, e = self._params.span(name)
                self._params.grad[s:e].zero_()
        self._counter_advanced = False
        self._pi_sampled = False
        self._train_policy(obs_list=obs_list, state=state, action=action, mu_d_policy_probs=mu_d_policy_probs)
        if self._auto_alpha():
            self._train_alpha(obs_list, state)
        if self.curiosity is not None:
            self._train_curiosity(n_padding_masks=n_padding_masks, nx_states=nx_states, n_actions=n_actions)
        if self.use_rnd:
            self._train_rnd(n_padding_masks=n_padding_masks, n_states=n_states, n_actions=n_actions)
        if not self._counter_advanced:
            self._steps_pi.add_(1)
        if self._summary_due():
            self._refresh_policy_stats()
            tags = {}
            if self.d_action_sizes and not self.discrete_dqn_like:
                tags['loss/d_entropy'] = self._stats['d_entropy']
                if self.use_auto_alpha:
                    tags['loss/d_alpha'] = torch.exp(self.log_d_alpha.detach())
            if self.c_action_size:
                tags['loss/c_entropy'] = self._stats['c_entropy']
                if self.use_auto_alpha:
                    tags['loss/c_alpha'] = torch.exp(self.log_c_alpha.detach())
            if self.curiosity is not None:
                tags['loss/curiosity'] = self._stats['loss_curiosity']
            self._write_option_summary(tags)

    # -- termination (option_base.py:675-717) ------------------------------------------------------------------------
    def compute_termination_grads(self, terminal_entropy, obs_list, state, y, v_over_options, done, priority_is):
        """Leaves d loss_termination / d (termination head) in the flat gradient buffer"""
        termination = self.model_termination(state.detach(), obs_list)                     # [batch, 1]
        B = termination.shape[0]
        dbeta = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.no_grad():
            native.termination_loss_grad(termination.detach(), y.detach(), v_over_options, done.contiguous(),
                                         priority_is, terminal_entropy, self._loss_termination, dbeta,
                                         workspace=self._termination_ws)
        self.optimizer_termination.zero_grad()
        with learner_backward():
            torch.autograd.backward([termination], [dbeta.view_as(termination)])
        if self._summary_due():
            self._stats['termination'].copy_(torch.mean(termination.detach()))
            self._write_option_summary({'loss/termination': self._stats['loss_termination'],
                                        'metric/termination': self._stats['termination']})

    def train_termination(self):
        self.optimizer_termination.step()

    # -- TD error (option_base.py:719-801) ---------------------------------------------------------------------------
    @torch.no_grad()
    def _get_td_error(self, next_n_vs_over_options, n_last_masks, n_padding_masks, nx_obses_list, nx_target_obses_list,
                      state, nx_target_states, n_actions, n_rewards, n_dones, n_mu_probs):
        """-> mean_e |Q_e(s_0, a_0) - y| [batch, 1]"""
        self._check_batch(n_rewards.shape[0])
        dsum = self.d_action_summed_size
        n_target_terminations = self._target_terminations(nx_target_states, nx_target_obses_list)
        obs_list = [o[:, 0] for o in nx_obses_list]
        action = n_actions[:, 0]
        d_action, c_action = action[..., :dsum], action[..., dsum:]
        B = state.shape[0]
        q_list = None
        if self.d_action_sizes:
            q_list = [q(state, c_action, obs_list) for q in self.model_q_list]
            c_q = torch.stack([q[1] for q in q_list]).squeeze(-1).contiguous() if self.c_action_size else None
        else:
            c_q = self._c_q_values(False, state, c_action, obs_list).contiguous()
        fused_d = self._option_discrete_fused(B, next_n_vs_over_options.shape[-1])
        fused_td = fused_d or (bool(self.c_action_size) and not self.d_action_sizes)
        td = torch.empty(B, dtype=torch.float32, device=self.device)
        d_y, c_y = self._get_y(next_n_vs_over_options, n_target_terminations, n_last_masks, n_padding_masks,
                               nx_obses_list, nx_target_states, n_actions, n_rewards, n_dones,
                               n_mu_probs if self.use_n_step_is else None,
                               eps_buf=self._eps_td, subset_prefix='td',
                               q_online=c_q if fused_td and not fused_d else None, td_out=td,
                               d_q_online=[q[0] for q in q_list] if fused_d else None)
        if fused_td:
            return td.unsqueeze(-1)
        err = torch.zeros((self.ensemble_q_num, B, 1), device=self.device)
        if self.d_action_sizes:
            d_q = torch.stack([torch.sum(d_action * q[0], dim=-1, keepdim=True) / self.d_action_branch_size
                               for q in q_list])
            err = err + torch.abs(d_q - d_y)
        if self.c_action_size:
            err = err + torch.abs(c_q.unsqueeze(-1) - c_y)
        return err.mean(dim=0)

    def _check_batch(self, rows: int) -> None:
        """the parent's policy / temperature steps work on static buffers of `batch_size` rows (noise, critic values,
        gradients): the training calls take exactly that many rows.  A selector whose options see varying numbers of rows
        pads or re-batches them; lifting this belongs with the selector"""
        if rows != self.batch_size:
            raise ValueError(f'OptionBase was built with batch_size={self.batch_size} and takes batches of that size, '
                             f'got {rows} rows')

    # -- checkpoint extras / summaries ---------------------------------------------------------------------------------
    def _summary_due(self) -> bool:
        return self.summary_writer is not None and self.get_global_step() % self.write_summary_per_step == 0

    def _write_option_summary(self, tags: dict) -> None:
        if not self._summary_due():
            return
        self.summary_available = True
        step = self.get_global_step()
        for tag, value in tags.items():
            self.summary_writer.add_scalar(tag, value, step)
        self.summary_writer.flush()
