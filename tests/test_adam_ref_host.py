"""CPU: the float64 restatement tests/test_adam_float64_gpu.py holds the Adam launches to (`adam_ref.step64`) is torch's own
Adam, not a copy of the kernels' formula; the workspace layout helper of the partials launch against a naive loop."""
import numpy as np
import torch

from tests import adam_ref as ar

EPS64 = 2.0 ** -52


def test_step64_is_torch_adam_in_float64():
    """every value case of the GPU test, from the same injected state, against `torch.optim.Adam(foreach=False)` run on
    the CPU in float64: per tensor within 16 float64 roundings at the tensor's largest magnitude (the two differ in the
    order of a handful of operations only)"""
    rng = np.random.default_rng(0)
    worst = 0.
    for done, scale, p_zero, hyper, all_zero in ar.value_cases():
        p, g, m, v = ar.make_state(rng, 257, done, scale, p_zero, all_zero)
        want = ar.step64(p, g, m, v, done + 1, *hyper)
        got = ar.torch_adam(p, g, m, v, done + 1, *hyper, torch.float64, 'cpu')
        for name, w_, g_ in zip(('param', 'exp_avg', 'exp_avg_sq'), want, got):
            assert w_.dtype == np.float64 and g_.dtype == np.float64 and np.isfinite(w_).all()
            size = np.abs(w_).max()
            err = np.abs(w_ - g_).max()
            assert err <= 16 * EPS64 * size, (name, done, scale, p_zero, hyper, err, size)
            worst = max(worst, err / (EPS64 * size) if size > 0 else 0.)
        if not all_zero:
            assert not np.array_equal(want[0], p.astype(np.float64)), 'the step moves the parameters'
    print(f'step64 against torch.optim.Adam in float64: at worst {worst:.2f} float64 roundings')


def test_step64_rounds_the_hyper_parameters_to_float32_first():
    p, g, m, v = (np.array([x], np.float32) for x in (0.5, 0.25, 0.1, 0.01))
    rounded = tuple(float(np.float32(x)) for x in ar.HYPER_DEFAULT)
    assert rounded != ar.HYPER_DEFAULT
    for a, b in zip(ar.step64(p, g, m, v, 10, *ar.HYPER_DEFAULT), ar.step64(p, g, m, v, 10, *rounded)):
        assert np.array_equal(a, b)


def test_partials_workspace_layout_against_a_triple_loop():
    rng = np.random.default_rng(1)
    for tiles, E, ms in ((1, 1, 5), (3, 2, 7), (17, 3, 5), (2, 3, 11)):
        partial = rng.standard_normal((tiles, E, ms)).astype(np.float32)
        loss = rng.standard_normal((tiles, E)).astype(np.float32)
        naive = np.full(tiles * E * ms + tiles * E, np.nan, np.float32)
        for t in range(tiles):
            for e in range(E):
                for local in range(ms):
                    naive[t * E * ms + e * ms + local] = partial[t, e, local]
                naive[tiles * E * ms + t * E + e] = loss[t, e]
        assert np.array_equal(ar.partials_workspace(partial, loss), naive)
        assert np.array_equal(ar.partials_workspace(partial), naive[:tiles * E * ms])


def test_partials_gradient_against_a_loop():
    """`partials_gradient` (numpy float64 and torch float32 forms) against the kernel's rule written out per element"""
    rng = np.random.default_rng(2)
    for tiles, E, ms, used, accumulate in ((3, 2, 7, 4, 0), (3, 2, 7, 4, 1), (1, 1, 5, 5, 1), (17, 3, 5, 2, 0)):
        partial = rng.standard_normal((tiles, E, ms)).astype(np.float32).astype(np.float64)
        grad = rng.standard_normal(E * ms).astype(np.float32).astype(np.float64)
        naive = grad.copy()
        for e in range(E):
            for local in range(used):
                s = sum(partial[t, e, local] for t in range(tiles))
                naive[e * ms + local] = grad[e * ms + local] + s if accumulate else s
        got = ar.partials_gradient(np, partial, grad, used, accumulate)
        np.testing.assert_allclose(got, naive, rtol=0, atol=1e-14)
        got32 = ar.partials_gradient(torch, torch.from_numpy(partial).float(), torch.from_numpy(grad).float(), used, accumulate)
        np.testing.assert_allclose(got32.double().numpy(), naive, rtol=0, atol=1e-5)
        kept = np.arange(E * ms) % ms >= used
        assert np.array_equal(got[kept], grad[kept]) and np.array_equal(got32.double().numpy()[kept], grad[kept])
