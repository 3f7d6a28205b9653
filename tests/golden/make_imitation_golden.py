"""Mint the golden vectors of behaviour cloning (`algorithm/imitation_base.ImitationBase`) from the *reference*
implementation, run on the CPU.  Run where the reference tree is available (see make_golden.py):

    python tests/golden/make_imitation_golden.py [case names...]      (default: all)

  f14_imitation_<case>.npz   six `ImitationBase.train` steps on six episodes whose lengths cover two buckets and both
                             sides of a bucket edge: the initial weights (`w0/`), the episodes (`ep<i>/`), every step's loss
                             (`loss`), the first step's first moments (`g0/`, as the f6 fixtures name them), the
                             representation and policy weights after step 1 (`w_s1/`) and after step 6 (`w1/`; the
                             critics and the target networks keep their `w0/` values, which the maker asserts), Adam's
                             moments and step count after step 6 (`m6/`)
There is no `conv` case: with the 30 x 30 convolution plugin (tests/nn_conv_vanilla.py of the reference) the file is 2.5 MB,
1.6 MB with 8-bit frames and shorter episodes (the weights dominate), over the 1 MB limit of a committed fixture.
Fixtures are data only (inputs and expected outputs).
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg  # noqa: E402  (installs the reference shims)

from algorithm.imitation_base import ImitationBase  # noqa: E402
from algorithm.sac_base import SAC_Base  # noqa: E402
from algorithm.utils.enums import SEQ_ENCODER  # noqa: E402

EP_LENS = (5, 63, 64, 65, 130, 17)


def f14(case, nn_rel, sac_kw, d_action_sizes=(), c_action_size=2, obs_shapes=((6,),), obs_names=('vector',), seed=14):
    nn_mod = mg.load_ref_nn(nn_rel)
    mg.seed_all(seed)
    rng = np.random.default_rng(seed)
    sac = SAC_Base(obs_names=list(obs_names), obs_shapes=list(obs_shapes), d_action_sizes=list(d_action_sizes),
                   c_action_size=c_action_size, model_abs_dir=None, nn=nn_mod, device='cpu', batch_size=32, **sac_kw)
    imit = ImitationBase(sac)
    out = {}
    mods = {k: v for k, v in sac.ckpt_dict.items() if isinstance(v, torch.nn.Module)}

    def snapshot(prefix, only=None):
        for name, m in mods.items():
            if only is None or name in only:
                for k, v in m.state_dict().items():
                    out[f'{prefix}/{name}/{k}'] = v.numpy().copy()

    snapshot('w0')
    out['w0/log_d_alpha'] = sac.log_d_alpha.detach().numpy().copy()
    out['w0/log_c_alpha'] = sac.log_c_alpha.detach().numpy().copy()

    seen = {}
    orig_backward = torch.Tensor.backward

    def spy(t, *a, **k):
        seen['loss'] = float(t.detach())
        return orig_backward(t, *a, **k)

    params = imit.opt.param_groups[0]['params']
    n_rep = len(list(sac.model_rep.parameters()))
    losses = []
    for i, T in enumerate(EP_LENS):
        ep = mg.gen_episode(rng, obs_shapes, d_action_sizes, c_action_size, tuple(sac.seq_hidden_state_shape), T)
        for j, o in enumerate(ep['ep_obses_list']):
            out[f'ep{i}/obs_{j}'] = o
        for k in ('ep_actions', 'ep_rewards', 'ep_dones'):
            out[f'ep{i}/{k}'] = ep[k]
        torch.Tensor.backward = spy
        try:
            step = imit.train(ep['ep_obses_list'], ep['ep_actions'], ep['ep_rewards'], ep['ep_dones'])
        finally:
            torch.Tensor.backward = orig_backward
        assert step == i + 1
        assert np.isfinite(seen['loss']), (case, i, seen['loss'])
        losses.append(seen['loss'])
        if i == 0:
            snapshot('w_s1', only=('model_rep', 'model_policy'))
            for j, p in enumerate(params):      # the first step's first moment: (1 - beta1) * gradient
                oname, jj = ('optimizer_rep', j) if j < n_rep else ('optimizer_policy', j - n_rep)
                st = imit.opt.state.get(p)
                out[f'g0/{oname}/{jj}'] = (st['exp_avg'] if st else torch.zeros_like(p)).detach().numpy().copy()
    out['loss'] = np.array(losses, np.float64)
    out['n_episodes'] = np.int64(len(EP_LENS))
    snapshot('w1', only=('model_rep', 'model_policy'))
    # imitation trains the representation and the policy only: the critics' and the target networks' weights after
    # step 6 ARE their `w0/` entries (checked here, recorded once: the fixture stays under the size limit)
    for name, m in mods.items():
        if name not in ('model_rep', 'model_policy'):
            for k, v in m.state_dict().items():
                assert np.array_equal(out[f'w0/{name}/{k}'], v.numpy()), (name, k)
    out['others_unchanged'] = np.bool_(True)
    for j, p in enumerate(params):
        st = imit.opt.state.get(p)      # (none for a parameter the loss never reaches: the discrete head's — zeros)
        zero = np.zeros(tuple(p.shape), np.float32)
        out[f'm6/exp_avg/{j}'] = st['exp_avg'].detach().numpy().copy() if st else zero
        out[f'm6/exp_avg_sq/{j}'] = st['exp_avg_sq'].detach().numpy().copy() if st else zero
        if st:
            out['m6/step'] = np.int64(int(float(st['step'])))
    for k, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            assert np.isfinite(v).all(), (case, k)
    sac.close()
    path = HERE / f'f14_imitation_{case}.npz'
    np.savez_compressed(path, **out)
    assert path.stat().st_size < 1_000_000, (case, path.stat().st_size)
    print(case, 'losses', ' '.join(f'{x:.6f}' for x in losses), path.stat().st_size, 'bytes')


CASES = {
    'mlp': lambda: f14('mlp', 'envs/test/nn.py', {}),
    'rnn': lambda: f14('rnn', 'envs/test/nn_rnn.py', dict(seq_encoder=SEQ_ENCODER.RNN)),
    # (the reference's envs/test/nn_attn.py has an unbounded state: its imitation losses reach 1e17 within six steps; the
    # bounded-state plugin of this repository, plugin API only, is the well-conditioned ATTN case, as for f6_step_attn_tanh)
    'attn': lambda: f14('attn', str(HERE.parent / 'plugins' / 'nn_attn_tanh.py'), dict(seq_encoder=SEQ_ENCODER.ATTN)),
    'hybrid': lambda: f14('hybrid', 'envs/test/nn.py', {}, d_action_sizes=(3, 2)),
}


def main():
    torch.set_num_threads(1)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()


if __name__ == '__main__':
    main()
