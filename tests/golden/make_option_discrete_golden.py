"""Mint the golden vectors of a PURE-DISCRETE, policy-based option (`algorithm/oc/option_base.OptionBase` with discrete
branches alone and `discrete_dqn_like=False`: the shape of the reference's option-critic configurations) from the
*reference* implementation, run on the CPU.  Run where the reference tree is available (see make_golden.py):

    python tests/golden/make_option_discrete_golden.py [pd32 | pd4_n1 | get_y ...]      (default: all)

  f19_option_discrete_pd32.npz, f19_option_discrete_pd4_n1.npz
        make_option_golden.f15's full call sequence (same keys: `d_y`, `td_error`, `g0/`, `w_rq/`, `w_pi/`, `w_term/`,
        `perm/<i>`, ...) on tests/plugins/nn_oc_small.py
  f19_option_discrete_get_y.npz
        OptionBase._get_y with the policy and the target critics replaced by tables (as f15_option_get_y for the
        continuous branch): exactly the arithmetic of `asac_option_discrete_return`.  Per case `<tag>_`: `logits`
        [B, n+1, D] (the policy is one OneHotCategorical per branch over them), `q` [E, B, n+1, D], the call's arguments,
        the recorded `perm` draws (next subset first), `log_alpha`, `y`, `cfg` = (n, E, E_sample, IS), `sizes`, `params`.
Fixtures are data only (inputs, recorded draws, expected outputs).
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_option_golden as mog  # noqa: E402  (installs the reference shims)
import make_golden as mg  # noqa: E402
import ref_shims  # noqa: E402

from algorithm.nn_models.policy import JointOneHotCategorical  # noqa: E402

PREFIX = 'f19_option_discrete_'


def _f15_as(case, *args, **kw):
    """make_option_golden.f15 with its file written under this generator's name"""
    save = mog._save
    mog._save = lambda path, out: save(HERE / f'{PREFIX}{case}.npz', out)
    try:
        mog.f15(case, *args, **kw)
    finally:
        mog._save = save


def get_y():
    out = {}
    rng = np.random.default_rng(19)
    B = 21
    for tag, n, sizes, E, Es, use_is in [('n4_s32', 4, (3, 2), 2, 2, True), ('n3_s253_e4s2', 3, (2, 5, 3), 4, 2, True),
                                         ('n40_s4', 40, (4,), 2, 2, True), ('n1_s32_nois', 1, (3, 2), 2, 2, False)]:
        D = sum(sizes)
        opt = mog._option(mog.SMALL, n_step=n, d_action_sizes=list(sizes), c_action_size=0, ensemble_q_num=E,
                          ensemble_q_sample=Es, use_n_step_is=use_is, gamma=0.99, v_lambda=0.95, v_rho=1.0, v_c=0.9)
        logits = torch.from_numpy((rng.standard_normal((B, n + 1, D)) * 2).astype(np.float32))
        qtab = [torch.from_numpy(rng.standard_normal((B, n + 1, D)).astype(np.float32)) for _ in range(E)]
        policy = JointOneHotCategorical([torch.distributions.OneHotCategorical(logits=part, validate_args=False)
                                         for part in logits.split(list(sizes), dim=-1)])
        opt.model_policy = lambda states, obs: (policy, None)
        opt.model_target_q_list = [(lambda s, a, o, t=t: (t, None)) for t in qtab]
        with torch.no_grad():
            opt.log_d_alpha.fill_(float(rng.uniform(-3, 0)))
        args = dict(
            next_n_vs_over_options=rng.standard_normal((B, n, mog.O)).astype(np.float32),
            n_terminations=mog._betas(rng, (B, n)),
            n_last_masks=rng.random((B, n)) < 0.15, n_padding_masks=rng.random((B, n)) < 0.2,
            n_actions=np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, (B, n))] for s in sizes], -1),
            n_rewards=rng.standard_normal((B, n)).astype(np.float32),
            n_dones=rng.random((B, n)) < 0.3,
            n_mu_probs=(rng.random((B, n, D)) * 0.9 + 0.1).astype(np.float32))
        nx_states = torch.zeros((B, n + 1, 6))
        mg.seed_all(190 + n)
        with ref_shims.DrawRecorder() as rec, torch.no_grad():
            d_y, _ = opt._get_y(nx_obses_list=[nx_states], nx_states=nx_states,
                                **{k: torch.from_numpy(v.copy()) for k, v in args.items()})
        assert len(rec.perm) == 2 and not rec.eps
        for k, v in args.items():
            out[f'{tag}_{k}'] = v
        out[f'{tag}_logits'] = logits.numpy()
        out[f'{tag}_q'] = torch.stack(qtab).numpy()
        out[f'{tag}_perm'] = torch.stack(rec.perm).numpy()
        out[f'{tag}_log_alpha'] = opt.log_d_alpha.detach().numpy()
        out[f'{tag}_y'] = d_y.numpy()
        out[f'{tag}_cfg'] = np.array([n, E, Es, int(use_is)])
        out[f'{tag}_sizes'] = np.array(sizes)
        out[f'{tag}_params'] = np.array([0.99, 0.95, 1.0, 0.9])
    mog._save(HERE / f'{PREFIX}get_y.npz', out)


CASES = {
    'pd32': lambda: _f15_as('pd32', mog.SMALL, dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2, use_n_step_is=True,
                                                    **mog.IS), d_action_sizes=(3, 2), c_action_size=0),
    'pd4_n1': lambda: _f15_as('pd4_n1', mog.SMALL, dict(n_step=1, use_n_step_is=False), d_action_sizes=(4,),
                              c_action_size=0, with_is_weights=True),
    'get_y': get_y,
}


def main():
    torch.set_num_threads(1)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()


if __name__ == '__main__':
    main()
