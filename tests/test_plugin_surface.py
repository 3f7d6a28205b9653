"""CPU: the model-plugin surface (`import algorithm.nn_models as m`) is wide enough for the
reference's own plugin files.  The files themselves are read from /root/reference when it is present (this
container; skipped elsewhere — nothing of the reference travels); the import-path and augmentation checks
need no reference, and the configuration keys are read from a fixture (`golden/reference_config_keys.json`)."""
import glob
import importlib
import importlib.util
import os
from pathlib import Path

import pytest
import torch

import algorithm.nn_models as m

REF = Path('/root/reference')
# plugin files whose own imports need packages this image lacks (torchvision) or a parent package
# (`from .nn_low import ...`): not a property of the surface under test
_SKIP_IMPORT = ('No module named \'torchvision\'', 'attempted relative import')


def _plugin_files(*patterns):
    return sorted(f for p in patterns for f in glob.glob(str(REF / p)))


def _load(path):
    spec = importlib.util.spec_from_file_location('ref_plugin_' + Path(path).stem + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_module_paths_resolve():
    """names user files import by module path (`from algorithm.nn_models.layers.seq_layers import GATE`, …)"""
    for path, names in {
        'algorithm.nn_models.layers.seq_layers': ['GATE', 'POSITIONAL_ENCODING', 'GRU', 'MultiheadAttention',
                                                  'EpisodeMultiheadAttention'],
        'algorithm.nn_models.layers.linear_layers': ['LinearLayers'],
        'algorithm.nn_models.layers.image_layers': ['ConvLayers', 'Conv1dLayers', 'ConvTransposeLayers', 'Transform'],
        'algorithm.nn_models.q': ['ModelBaseQ', 'ModelQ'],
        'algorithm.nn_models.policy': ['ModelBasePolicy', 'ModelPolicy', 'ModelTermination'],
        'algorithm.nn_models.representation': ['ModelBaseRep', 'ModelSimpleRep', 'ModelBaseAttentionRep',
                                               'ModelBaseOptionSelectorRep', 'ModelVOverOptions',
                                               'ModelRepProjection', 'ModelRepPrediction'],
        'algorithm.nn_models.predictions': ['ModelTransition', 'ModelReward', 'ModelBaseObservation'],
        'algorithm.nn_models.exploration': ['ModelRND', 'ModelForwardDynamic', 'ModelInverseDynamic'],
        'algorithm.utils.transform': ['GaussianNoise', 'SaltAndPepperNoise', 'DepthNoise', 'DepthSaltAndPepperNoise'],
        'algorithm.utils.visualization.image': ['ImageVisual'],
        'algorithm.utils.visualization.ray': ['RayVisual'],
    }.items():
        mod = importlib.import_module(path)
        for n in names:
            assert hasattr(mod, n), f'{path}.{n}'
            if path.startswith('algorithm.nn_models'):
                assert getattr(m, n) is getattr(mod, n)


def test_noise_augmentations():
    from algorithm.utils.transform import DepthNoise, DepthSaltAndPepperNoise, GaussianNoise, SaltAndPepperNoise
    torch.manual_seed(0)
    img = torch.rand(4, 3, 16, 16)
    out = GaussianNoise(mean=0., std=.1)(img)
    assert out.shape == img.shape and out.min() >= 0 and out.max() <= 1
    assert torch.all(out >= img - 1e-6) and torch.all(out <= img + .1 + 1e-6)     # uniform noise in [0, std)
    out = SaltAndPepperNoise(snr=.3, p=.9)(img)
    changed = (out != img).any(dim=1)                                               # one draw per pixel, all channels
    assert 0.02 < changed.float().mean() < 0.2
    delta = (out - img)[changed.unsqueeze(1).expand_as(img)]
    assert torch.all((delta.abs() <= .3 + 1e-6))
    out = DepthNoise(.2)(img)
    d = out - img
    inside = (out > 0) & (out < 1)
    assert torch.allclose(d[inside], d[inside][0].expand_as(d[inside]), atol=1e-6)  # one offset for the batch
    out = DepthSaltAndPepperNoise(snr=1., p=.5)(img)
    assert set(out[out != img].unique().tolist()) <= {0., 1.}
    with pytest.raises(TypeError):
        GaussianNoise()(img.numpy())
    assert m.Transform(GaussianNoise())(img.unsqueeze(1)).shape == (4, 1, 3, 16, 16)


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present or not readable')
def test_reference_plugin_files_import():
    files = _plugin_files('envs/*/nn*.py', 'envs/*/*/nn*.py', 'tests/nn*.py')
    assert len(files) > 40
    imported = 0
    for f in files:
        try:
            mod = _load(f)
        except (ImportError, ModuleNotFoundError) as e:
            assert any(s in str(e) for s in _SKIP_IMPORT), f'{f}: {e}'
            continue
        imported += 1
        assert any(hasattr(mod, n) for n in ('ModelRep', 'ModelOptionSelectorRep', 'ModelQ', 'ModelPolicy')), f
    assert imported >= 45


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present or not readable')
@pytest.mark.parametrize('rel', ['envs/test/nn.py', 'envs/test/nn_rnn.py', 'envs/test/nn_attn.py',
                                 'tests/nn_conv_vanilla.py', 'tests/nn_conv_rnn.py', 'tests/nn_conv_attn.py'])
def test_reference_test_plugins_build_and_run(rel):
    """the plugin files the BASELINE configurations name: constructed with the learner's argument order
    (sac_base.py:340-345, 396-400, 416-418) and run over a [batch, L] window on the module path"""
    mod = _load(str(REF / rel))
    shapes = [(6,)] if rel.startswith('envs/test') else [(10,), (3, 30, 30)]
    names = ['vector', 'image'][:len(shapes)]
    B, L, A = 2, 4, 3
    torch.manual_seed(0)
    rep = mod.ModelRep(names, shapes, [], A, False)
    obs = [torch.randn(B, L, *s) for s in shapes]
    pre_action, pad = torch.randn(B, L, A), torch.zeros(B, L, dtype=torch.bool)
    if isinstance(rep, m.ModelBaseAttentionRep):
        index = torch.arange(L).unsqueeze(0).repeat(B, 1)
        state, hidden, *_ = rep(L, index, obs, pre_action, None, padding_mask=pad)
    else:
        state, hidden = rep(obs, pre_action, None, padding_mask=pad)
    assert state.shape[:2] == (B, L) and hidden.shape[:2] == (B, L) and torch.isfinite(state).all()
    S = state.shape[-1]
    q = mod.ModelQ(S, [], A, False)
    _, c_q = q(state, torch.randn(B, L, A), obs)
    assert c_q.shape == (B, L, 1)
    d_policy, c_policy = mod.ModelPolicy(S, [], A)(state, obs)
    assert d_policy is None and c_policy.rsample().shape == (B, L, A)
    if list(rep.parameters()):
        state.sum().backward()
        assert all(p.grad is not None for p in rep.parameters() if p.requires_grad)


def test_every_reference_config_key_is_accepted():
    """every `sac_config` / `replay_config` key of the reference's default and per-environment YAML files is a
    keyword of `SAC_Base` / `PrioritizedReplayBuffer` (sac_base.py:22-93, replay_buffer.py:246-258), including the
    per-agent override sections (`ma_config`).  The keys, file by file: `golden/reference_config_keys.json`
    (`golden/make_config_keys.py`)."""
    import inspect
    import json

    from algorithm.replay_buffer import PrioritizedReplayBuffer
    from algorithm.sac_base import SAC_Base
    sac_kw = set(inspect.signature(SAC_Base.__init__).parameters)
    replay_kw = set(inspect.signature(PrioritizedReplayBuffer.__init__).parameters)
    files = json.loads((Path(__file__).resolve().parent / 'golden' / 'reference_config_keys.json').read_text())
    assert len(files) > 20 and 'algorithm/default_config.yaml' in files
    seen = set()
    for where, keys in files.items():
        unknown = set(keys['sac_config']) - sac_kw
        assert not unknown, f'{where}: sac_config keys {unknown}'
        unknown = set(keys['replay_config']) - replay_kw
        assert not unknown, f'{where}: replay_config keys {unknown}'
        seen.update(keys['sac_config'])
    assert {'n_step', 'burn_in_step', 'seq_encoder', 'curiosity', 'siamese', 'use_rnd'} <= seen
