"""Mint the golden vectors of the training mode without a replay buffer (`use_replay_buffer=False`) from the
*reference* implementation.  Run where the reference tree is available (see make_golden.py):

    python tests/golden/make_batch_golden.py [fixture function names...]      (default: all)

  f12_batch_buffer.npz     the reference BatchBuffer driven by a put / get script: every permutation it drew, every
                           batch it returned (rest carry-over, an exact multiple, a queue overflow, empty gets,
                           burn-in 2 / n_step 3, -1 indexes inside an episode, an 8-bit image key, a hidden state)
  f13_batch_step_<case>.npz  full reference train() steps with use_replay_buffer=False: weights before / after,
                           episodes, the batch permutations, the step's draws, its losses / entropies / temperature
Fixtures are data only (inputs, recorded random draws, expected outputs).
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg  # noqa: E402  (installs the reference shims)
import ref_shims  # noqa: E402

from algorithm.batch_buffer import BatchBuffer  # noqa: E402
from algorithm.sac_base import SAC_Base  # noqa: E402
from algorithm.utils.enums import SEQ_ENCODER  # noqa: E402


class PermutationRecorder:
    """records every `np.random.permutation(n)` drawn while active"""

    def __init__(self):
        self.perms = []

    def __enter__(self):
        self._orig = np.random.permutation
        rec = self

        def perm(n):
            p = rec._orig(n)
            rec.perms.append(np.asarray(p).copy())
            return p

        np.random.permutation = perm
        return self

    def __exit__(self, *exc):
        np.random.permutation = self._orig


# ------------------------------------------------------------------------------------------------
F12 = dict(burn_in=2, n_step=3, batch_size=8, max_size=10, A=2, hidden=(5,), img=(2, 3, 4))
# the script: ('put', episode length, indexes set to -1) | ('get', count)
F12_SCRIPT = [('put', 13, ()), ('get', 1), ('put', 21, ()), ('get', 4), ('put', 7, (2, 3)), ('put', 120, (50,)),
              ('get', 3), ('put', 30, ()), ('get', 12)]


def f12_episode(rng, e, T, minus_one):
    """vector observation channel 0 = 1000 e + t: the (episode, start) identity of a window is its row `burn_in`"""
    vec = rng.standard_normal((1, T, 4)).astype(np.float32)
    vec[0, :, 0] = 1000 * e + np.arange(T)
    idx = np.arange(T, dtype=np.int32)[None]
    idx[0, list(minus_one)] = -1
    return dict(
        ep_indexes=idx,
        ep_obses_list=[vec, rng.integers(0, 256, (1, T, *F12['img'])).astype(np.uint8)],
        ep_actions=rng.random((1, T, F12['A'])).astype(np.float32),
        ep_rewards=rng.standard_normal((1, T)).astype(np.float32),
        ep_dones=(rng.random((1, T)) < 0.3),
        ep_probs=rng.random((1, T, F12['A'])).astype(np.float32),
        ep_pre_seq_hidden_states=rng.standard_normal((1, T, *F12['hidden'])).astype(np.float32))


def last_masks(ep_indexes):
    last = np.zeros_like(ep_indexes, dtype=bool)      # SAC_Base.put_episode (reference sac_base.py:2326-2328)
    last[:, -1] = True
    last[ep_indexes == -1] = True
    return last


BATCH_KEYS = ('bn_indexes', 'bn_last_masks', 'bn_padding_masks', 'bnx_obses', 'bn_actions', 'bn_rewards', 'bn_dones',
              'bn_probs', 'bnx_pre_seq_hidden_states')


def f12_batch_buffer():
    mg.seed_all(12)
    rng = np.random.default_rng(12)
    c = F12
    pad = np.array([0.25, -0.5], np.float32)
    bb = BatchBuffer(burn_in_step=c['burn_in'], n_step=c['n_step'], padding_action=pad, batch_size=c['batch_size'],
                     max_size=c['max_size'])
    out = {k: np.int64(v) for k, v in c.items() if isinstance(v, int)}
    out['hidden'], out['img'] = np.array(c['hidden']), np.array(c['img'])
    out['padding_action'] = pad
    ops, n_put, n_get = [], 0, 0
    for op in F12_SCRIPT:
        if op[0] == 'put':
            _, T, minus_one = op
            ep = f12_episode(rng, n_put, T, minus_one)
            for k, v in ep.items():
                if k == 'ep_obses_list':
                    for j, o in enumerate(v):
                        out[f'put{n_put}/obs_{j}'] = o
                else:
                    out[f'put{n_put}/{k}'] = v
            with PermutationRecorder() as rec:
                bb.put_episode(ep_last_masks=last_masks(ep['ep_indexes']), **ep)
            assert len(rec.perms) == 1
            out[f'put{n_put}/perm'] = rec.perms[0].astype(np.int64)
            ops.append(0)
            n_put += 1
        else:
            for _ in range(op[1]):
                batch = bb.get_batch()
                out[f'get{n_get}/empty'] = np.bool_(batch is None)
                if batch is not None:
                    for k, v in zip(BATCH_KEYS, batch):
                        if k == 'bnx_obses':
                            for j, o in enumerate(v):
                                out[f'get{n_get}/obs_{j}'] = o.numpy()
                        else:
                            out[f'get{n_get}/{k}'] = v.numpy()
                    ident = batch[3][0][:, c['burn_in'], 0].numpy().astype(np.int64)
                    out[f'get{n_get}/windows'] = np.stack([ident // 1000, ident % 1000], 1)
                ops.append(1)
                n_get += 1
    out['ops'] = np.array(ops, np.int64)
    out['n_put'], out['n_get'] = np.int64(n_put), np.int64(n_get)
    np.savez_compressed(HERE / 'f12_batch_buffer.npz', **out)


# ------------------------------------------------------------------------------------------------
def f13_step(case, nn_rel, sac_kw, ep_lens, n_steps, obs_shapes=((6,),), obs_names=('vector',), c_action_size=2,
             seed=13, final_weights=True):
    """`final_weights=False`: no `w1/` and `g0/` entries (keeps a convolution case under the fixture size limit; its
    losses, entropy and temperature, and the representation / critic weights right after their update, still pin it)"""
    nn_mod = mg.load_ref_nn(nn_rel)
    mg.seed_all(seed)
    rng = np.random.default_rng(seed)
    sac = SAC_Base(obs_names=list(obs_names), obs_shapes=list(obs_shapes), d_action_sizes=[], c_action_size=c_action_size,
                   model_abs_dir=None, nn=nn_mod, device='cpu', use_replay_buffer=False, **sac_kw)
    out = {}
    mods = {k: v for k, v in sac.ckpt_dict.items() if isinstance(v, torch.nn.Module)}
    for name, m in mods.items():
        for k, v in m.state_dict().items():
            out[f'w0/{name}/{k}'] = v.numpy().copy()
    out['w0/log_d_alpha'] = sac.log_d_alpha.detach().numpy().copy()
    out['w0/log_c_alpha'] = sac.log_c_alpha.detach().numpy().copy()
    for i, T in enumerate(ep_lens):
        ep = mg.gen_episode(rng, obs_shapes, (), c_action_size, tuple(sac.seq_hidden_state_shape), T)
        recorded = dict(ep, ep_obses_list=list(ep['ep_obses_list']))   # (episode_to_batch pads the list in place)
        with PermutationRecorder() as rec:
            sac.put_episode(**ep)
        out[f'ep{i}/perm'] = rec.perms[0].astype(np.int64)
        for k, v in recorded.items():
            if k == 'ep_obses_list':
                for j, o in enumerate(v):
                    if o.ndim == 5:
                        u8 = np.rint(o * 255.).astype(np.uint8)
                        assert np.array_equal(u8.astype(np.float32) / np.float32(255.), o)
                        out[f'ep{i}/obs_{j}_u8'] = u8
                    else:
                        out[f'ep{i}/obs_{j}'] = o
            else:
                out[f'ep{i}/{k}'] = v
    out['n_episodes'] = np.int64(len(ep_lens))

    seen = {}
    orig_rq, orig_pol = sac._train_rep_q, sac._train_policy
    rep_trains = any(p.requires_grad for p in sac.model_rep.parameters())

    def rq(*a, **k):
        r = orig_rq(*a, **k)
        seen['loss_q'] = r[0].detach().numpy().copy()
        if rep_trains:
            for name, m in mods.items():
                if name == 'model_rep' or name.startswith('model_q_'):
                    for kk, v in m.state_dict().items():
                        seen[f'w_rq/{name}/{kk}'] = v.numpy().copy()
        return r

    def pol(*a, **k):
        orig_backward = torch.Tensor.backward

        def spy(t, *ba, **bk):
            seen.setdefault('loss_policy', t.detach().numpy().copy())
            return orig_backward(t, *ba, **bk)

        torch.Tensor.backward = spy
        try:
            r = orig_pol(*a, **k)
        finally:
            torch.Tensor.backward = orig_backward
        seen['c_ent'] = None if r[1] is None else r[1].detach().numpy().copy()
        return r

    sac._train_rep_q, sac._train_policy = rq, pol
    for s in range(n_steps):
        seen.clear()
        with ref_shims.DrawRecorder() as rec:
            step = sac.train()
        assert step == s + 1, (step, s)
        assert not rec.u, 'batch mode draws no PER uniforms'
        for j, e in enumerate(rec.eps):
            out[f'step{s}/eps{j}'] = e.numpy()
        out[f'step{s}/n_eps'] = np.int64(len(rec.eps))
        out[f'step{s}/perm'] = (torch.stack(rec.perm).numpy() if rec.perm else np.zeros((0, 0), np.int64))
        out[f'step{s}/loss_q'] = seen['loss_q']
        out[f'step{s}/loss_policy'] = seen['loss_policy']
        if s == 0 and final_weights:
            for oname, opt in sac.ckpt_dict.items():
                if oname.startswith('optimizer') and opt is not None:
                    for j, p in enumerate(opt.param_groups[0]['params']):
                        st = opt.state.get(p)
                        if st:
                            out[f'g0/{oname}/{j}'] = st['exp_avg'].detach().numpy().copy()
        if seen.get('c_ent') is not None:
            out[f'step{s}/c_entropy'] = seen['c_ent']
        out[f'step{s}/log_c_alpha'] = sac.log_c_alpha.detach().numpy().copy()
        for kk, v in seen.items():
            if kk.startswith('w_rq/'):
                out[f'step{s}/{kk}'] = v
    for name, m in mods.items():
        for k, v in m.state_dict().items():
            if final_weights:
                out[f'w1/{name}/{k}'] = v.numpy().copy()
    out['n_steps'] = np.int64(n_steps)
    out['queued_after'] = np.int64(len(sac.batch_buffer._batch_list))
    sac.close()
    np.savez_compressed(HERE / f'f13_batch_step_{case}.npz', **out)


def f13_cases():
    vec = dict(batch_size=32)
    f13_step('n1', 'envs/test/nn.py', dict(n_step=1, use_priority=False, **vec), [60, 45, 70], 3)
    f13_step('n4_is', 'envs/test/nn.py', dict(n_step=4, use_priority=True, use_n_step_is=True, **vec), [60, 45, 70], 3)
    f13_step('rnn', 'envs/test/nn_rnn.py', dict(n_step=3, burn_in_step=3, seq_encoder=SEQ_ENCODER.RNN, **vec),
             [60, 45, 70], 3)
    f13_step('conv', 'tests/nn_conv_vanilla.py', dict(batch_size=8, burn_in_step=5, n_step=3, ensemble_q_num=4,
                                                      ensemble_q_sample=2), [14, 12], 1, final_weights=False, **mg.IMG_OBS)


def main():
    torch.set_num_threads(1)
    if len(sys.argv) > 1:
        for name in sys.argv[1:]:
            globals()[name]()
        return
    f12_batch_buffer()
    f13_cases()
    print('golden fixtures written to', HERE)


if __name__ == '__main__':
    main()
