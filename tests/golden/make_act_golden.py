"""Mint the fixture of policy-based acting from the *reference* implementation's own `_choose_action` (through
`choose_action`), in the mode that has no draws: `disable_sample=True`, `action_noise=None`.

Run where the reference tree is importable (see `make_golden.py`):   python tests/golden/make_act_golden.py
It writes, next to this file,
  f20_act.npz   per case: the weights of the representation and the policy (`<case>/w0/...`), the inputs
                (`<case>/in/...`), and `<case>/action`, `<case>/prob`, `<case>/hidden` as the reference returned them

`CASES` is what the tests read (tests/test_act_host.py, tests/test_act_gpu.py).  The policy's heads are kept narrow
(one 16-wide block each): the fixture is about the arithmetic behind the heads and stays a few KB.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
PLUGINS = HERE.parent / 'plugins'
N_ENV = 7
NARROW = {'policy': dict(d_dense_n=16, d_dense_depth=1, c_dense_n=16, c_dense_depth=1)}
# case -> (plugin, d_action_sizes, c_action_size, learner keywords)
CASES = {
    'discrete': ('nn_vec', (3, 2), 0, dict(n_step=3, nn_config=NARROW)),
    'hybrid': ('nn_vec', (3, 2), 2, dict(n_step=3, nn_config=NARROW)),
    'discrete_rnn': ('nn_rnn', (3, 2), 0, dict(n_step=3, burn_in_step=3, seq_encoder='RNN', nn_config=NARROW)),
}
SAVED = ('model_rep', 'model_policy')
SEED = 200


def main():
    sys.path.insert(0, str(HERE))
    import torch
    import make_golden as mg
    from algorithm.utils.enums import convert_config_to_enum
    torch.set_num_threads(1)
    out = {}
    for c, (case, (plugin, sizes, A, kw)) in enumerate(CASES.items()):
        kw = dict(kw)
        convert_config_to_enum(kw)
        mg.seed_all(SEED + c)
        rng = np.random.default_rng(SEED + c)
        sac = mg._tiny_sac(mg.load_ref_nn(str(PLUGINS / f'{plugin}.py')), d_action_sizes=list(sizes), c_action_size=A, **kw)
        gen = torch.Generator().manual_seed(SEED + c)
        for name in SAVED:
            if name not in sac.ckpt_dict:         # (a representation without parameters)
                continue
            for k, p in sac.ckpt_dict[name].state_dict().items():
                if k.endswith('bias'):        # the stock initialisation leaves the biases zero: give them values
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen))
                out[f'{case}/w0/{name}/{k}'] = p.detach().numpy().copy()
        D = sum(sizes)
        pre = np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, N_ENV)] for s in sizes]
                             + ([rng.random((N_ENV, A)).astype(np.float32)] if A else []), axis=-1)
        args = dict(obs_list=[rng.standard_normal((N_ENV, 6)).astype(np.float32)], pre_action=pre,
                    pre_seq_hidden_state=rng.standard_normal((N_ENV, *sac.seq_hidden_state_shape)).astype(np.float32))
        assert sac.action_noise is None
        action, prob, hidden = sac.choose_action([args['obs_list'][0].copy()], args['pre_action'].copy(),
                                                 args['pre_seq_hidden_state'].copy(), disable_sample=True)
        assert action.shape == prob.shape == (N_ENV, D + A)
        out[f'{case}/in/obs_list'], out[f'{case}/in/pre_action'] = args['obs_list'][0], args['pre_action']
        out[f'{case}/in/pre_seq_hidden_state'] = args['pre_seq_hidden_state']
        out[f'{case}/action'], out[f'{case}/prob'], out[f'{case}/hidden'] = action, prob, hidden
        sac.close()
    out['torch_version'] = np.array(torch.__version__)
    np.savez_compressed(HERE / 'f20_act.npz', **out)
    size = (HERE / 'f20_act.npz').stat().st_size
    assert size < 100_000, size
    print('f20_act', size, 'bytes')


if __name__ == '__main__':
    main()
