"""GPU: `asac_image_augment` (csrc/image.hip) behind `algorithm/utils/image_transforms.py` — each op against the float64
definitions of tests/image_ref.py, the device draws eager and inside a captured step, and the learner on
tests/plugins/nn_views.py.

Tolerances: blur and resize are compared with the float64 definition, never with the kernel itself or
the float32 module code, at 4x the largest error observed on the MI355X (tests/image_transform_tolerances.json, one figure
per case, written by `measure_errors` below).  The recorded figures must themselves stay under ceilings derived from the
arithmetic — blur 1e-5 absolute: at most 83 roundings of terms whose weights sum to 1, on values <= 1; resize 5e-5
absolute: float32 source coordinates up to 84 carry about 1e-5 of error per axis into the interpolation weight, times value
differences <= 1.  A figure over its ceiling is a bug, not a tolerance.  Crop alone, a resize to the same size and brightness
are bit-exact (the library is built with -ffp-contract=off)."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import asac_amd  # noqa: E402,F401
from algorithm.utils import image_transforms as T  # noqa: E402
from algorithm.utils.transform import GaussianNoise, SaltAndPepperNoise  # noqa: E402
import algorithm.nn_models as m  # noqa: E402
from asac_amd import native  # noqa: E402
from tests import image_ref as ref  # noqa: E402
from tests import parity_utils as pu  # noqa: E402

DEV = torch.device('cuda', 0)
TOLERANCES = Path(__file__).resolve().parent / 'image_transform_tolerances.json'
CEILING = {'blur': 1e-5, 'resize': 5e-5}


def _img(*shape, seed=0, lo=0., hi=1.):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo).to(DEV)


def _launches(fn):
    """-> (fn's result, the asac_* launches the profiler saw during it)"""
    with native.LaunchProfiler(repeat=1) as prof:
        out = fn()
    return out, prof.summary()


def _native(module, x):
    """module(x) and proof that it was ONE launch of the kernel"""
    out, seen = _launches(lambda: module(x))
    assert list(seen) == ['asac_image_augment'] and seen['asac_image_augment']['calls'] == 1, seen
    return out


# ---------------------------------------------------------------------------------------------- blur, resize
# name -> (input shape, kernel_size, sigma, how the input is handed over)
BLUR_CASES = {
    'reach_9x9_k9': ((1, 3, 9, 9), 9, 2.0, None),                # the reflection reaches the far side
    'pair_11x7_k5x3': ((2, 2, 11, 7), (5, 3), 0.8, None),        # H = 11, W = 7, (kx, ky) = (5, 3)
    'usv_84_k9_s9': ((2, 3, 84, 84), 9, 9.0, None),
    'plugin_30x30x6': ((1, 6, 30, 30), 9, 9.0, None),
    'one_channel': ((3, 1, 10, 12), 3, 1.5, None),
    'odd_planes': ((1, 5, 7, 9), 5, 1.0, None),                  # 5 planes of 63 floats: three of four are misaligned
    'lead_dims': ((2, 3, 2, 8, 8), 3, 0.6, None),                # [B, T, C, H, W]
    'non_contiguous': ((2, 3, 12, 10), 5, 1.2, 'transposed'),
    'k31': ((1, 1, 16, 40), (31, 1), 6.0, None),                 # the widest kernel
}
# name -> ((H, W), (Ho, Wo))
RESIZE_CASES = {'50_to_84': ((50, 50), (84, 84)), '7x5_to_7x9': ((7, 5), (7, 9)), '1x1_to_4x4': ((1, 1), (4, 4))}


def _blur_run(name):
    shape, k, sigma, how = BLUR_CASES[name]
    x = _img(*shape, seed=len(name))
    if how == 'transposed':
        x = _img(*shape[:-2], shape[-1], shape[-2], seed=len(name)).transpose(-1, -2)
        assert not x.is_contiguous()
    out = _native(T.GaussianBlur(k, sigma=sigma), x)
    kx, ky = (k, k) if isinstance(k, int) else k
    assert out.shape == x.shape and out.dtype == torch.float32
    return float(np.abs(out.double().cpu().numpy() - ref.blur(x.double().cpu().numpy(), kx, ky, sigma)).max())


def _resize_run(name):
    (H, W), (Ho, Wo) = RESIZE_CASES[name]
    x = _img(2, 3, H, W, seed=H)
    out = _native(T.Resize((Ho, Wo)), x)
    assert out.shape == (2, 3, Ho, Wo)
    return float(np.abs(out.double().cpu().numpy() - ref.resize(x.double().cpu().numpy(), Ho, Wo)).max())


def measure_errors():
    """what tests/image_transform_tolerances.json records: max |kernel - float64 definition| per case"""
    return {'device': torch.cuda.get_device_name(0),
            'blur': {n: _blur_run(n) for n in BLUR_CASES}, 'resize': {n: _resize_run(n) for n in RESIZE_CASES}}


def _bound(kind, name):
    recorded = json.loads(TOLERANCES.read_text())[kind][name]
    assert recorded <= CEILING[kind], f'{kind}/{name}: the recorded {recorded:.3g} is over the derived ceiling: a bug'
    # (an error of 0 on the recorded box leaves one float32 rounding at 1.0 as the bound)
    return 4 * max(recorded, 2. ** -24)


@pytest.mark.parametrize('name', list(BLUR_CASES))
def test_blur_against_the_float64_definition(name):
    err = _blur_run(name)
    print(f'blur/{name}: {err:.3g}')
    assert err <= _bound('blur', name)


@pytest.mark.parametrize('name', list(RESIZE_CASES))
def test_resize_against_the_float64_definition(name):
    err = _resize_run(name)
    print(f'resize/{name}: {err:.3g}')
    assert err <= _bound('resize', name)


def test_drawn_sigma_is_what_the_kernel_blurred_with():
    x = _img(1, 2, 12, 12, seed=5)
    blur = T.GaussianBlur(5, sigma=(0.5, 3.0)).reseed(11)
    sigmas = set()
    for call in range(6):
        out = _native(blur, x)
        d = blur.drawn()
        assert d['counter'] == call and 0.5 <= d['sigma'] < 3.0 and math.isnan(d['factor']) and d['top'] == -1
        want = ref.blur(x.double().cpu().numpy(), 5, 5, d['sigma'])
        assert np.abs(out.double().cpu().numpy() - want).max() <= CEILING['blur']
        sigmas.add(d['sigma'])
    assert len(sigmas) == 6


# ---------------------------------------------------------------------------------------------- crop, brightness
def test_crop_alone_is_the_slice_at_the_drawn_offsets():
    x = _img(2, 3, 9, 11, seed=1)
    crop = T.RandomCrop((5, 4)).reseed(3)
    seen = set()
    for _ in range(24):
        out = _native(crop, x)
        d = crop.drawn()
        assert 0 <= d['top'] <= 4 and 0 <= d['left'] <= 7
        assert torch.equal(out, x[..., d['top']:d['top'] + 5, d['left']:d['left'] + 4])
        seen.add((d['top'], d['left']))
    assert len(seen) >= 10                                     # 24 draws over 40 offsets
    assert torch.equal(_native(T.RandomCrop((9, 11)), x), x)   # the whole frame: nothing to draw


def test_resize_to_the_same_size_copies_the_bits():
    x = _img(2, 3, 7, 9, seed=2)
    x[0, 0, 0, 0], x[1, 2, 6, 8] = float('inf'), float('nan')
    out = _native(T.Resize((7, 9)), x)
    assert out.data_ptr() != x.data_ptr() and torch.equal(out.view(torch.int32), x.view(torch.int32))


def test_crop_then_resize_is_one_launch():
    x = _img(2, 3, 30, 30, seed=3)
    pair = T.Compose([T.RandomCrop(18), T.Resize((30, 30))]).reseed(5)
    out = _native(pair, x)
    d = pair.drawn()
    window = x[..., d['top']:d['top'] + 18, d['left']:d['left'] + 18].double().cpu().numpy()
    assert np.abs(out.double().cpu().numpy() - ref.resize(window, 30, 30)).max() <= CEILING['resize']


def test_a_downscale_runs_the_module_code():
    x = _img(1, 3, 16, 16, seed=4)
    out, seen = _launches(lambda: T.Resize((8, 8))(x))
    assert not [k for k in seen if k.startswith('asac_image_')], seen
    want = torch.nn.functional.interpolate(x, size=(8, 8), mode='bilinear', align_corners=False, antialias=True)
    assert torch.equal(out, want)
    # so do a plane over the cap, a blur that reaches past the plane, another dtype and an input that requires grad
    for module, inp in ((T.ColorJitter(brightness=(0.5, 0.5)), _img(1, 1, 97, 96)),
                        (T.ColorJitter(brightness=(0.5, 0.5)), _img(1, 1, 8, 8).double()),
                        (T.ColorJitter(brightness=(0.5, 0.5)), _img(1, 1, 8, 8).requires_grad_())):
        out, seen = _launches(lambda: module(inp))
        assert not seen and torch.equal(out, (inp * 0.5).clamp(0, 1))
    with pytest.raises(RuntimeError):
        T.GaussianBlur(9, sigma=1.)(_img(1, 1, 4, 12))


def test_brightness_is_bit_exact():
    x = _img(3, 3, 9, 7, seed=6) * 1.5
    x[0, 0, 0, 0] = float('nan')
    fixed = _native(T.ColorJitter(brightness=(1.3, 1.3)), x)
    assert torch.equal(fixed.view(torch.int32), (x * 1.3).clamp(0, 1).view(torch.int32))
    jitter = T.ColorJitter(brightness=0.4).reseed(9)
    factors = set()
    for _ in range(6):
        out = _native(jitter, x)
        f = jitter.drawn()['factor']
        assert 0.6 <= f <= 1.4 and float(np.float32(f)) == f
        assert torch.equal(out.view(torch.int32), (x * f).clamp(0, 1).view(torch.int32))
        factors.add(f)
    assert len(factors) == 6


# ---------------------------------------------------------------------------------------------- noise ops
def _noise_input():
    return _img(8, 3, 30, 30, seed=7, lo=0.3, hi=0.7)


def test_salt_and_pepper():
    x = _noise_input()
    sp = T.RandomChoice([m.Transform(SaltAndPepperNoise(0.2, 0.5))]).reseed(21)
    out = _native(sp, x)
    diff = (out - x).cpu()
    changed = diff != 0
    n = 8 * 30 * 30
    # every channel of a pixel changed together, by the same sign
    assert torch.equal(changed[:, 0], changed[:, 1]) and torch.equal(changed[:, 0], changed[:, 2])
    assert torch.equal(diff[:, 0] > 0, diff[:, 1] > 0) and torch.equal(diff[:, 0] > 0, diff[:, 2] > 0)
    frac = changed[:, 0].float().mean().item()
    assert abs(frac - 0.5) <= 0.035, frac                                   # 6 sigma of 7 200 draws
    # every changed pixel moved by exactly +-0.2 within float32 rounding of x +- 0.2 (|values| < 1: half an ulp is 2^-25)
    assert ((diff[changed].abs() - 0.2).abs() <= 2. ** -23).all()
    sigma = math.sqrt(0.25 * 0.75 / n)
    up, down = (diff[:, 0] > 0).float().mean().item(), (diff[:, 0] < 0).float().mean().item()
    assert abs(up - 0.25) <= 6 * sigma and abs(down - 0.25) <= 6 * sigma, (up, down)
    # the arithmetic is transform.py's: the same bits as its chained `where`s would give for these draws
    want = torch.where(diff > 0, (x.cpu() + 0.2).clamp(0, 1), torch.where(diff < 0, (x.cpu() - 0.2).clamp(0, 1), x.cpu()))
    assert torch.equal(out.cpu(), want)


def test_uniform_noise():
    x = _noise_input()
    noise = T.RandomChoice([GaussianNoise(0., 0.1)]).reseed(22)
    out = _native(noise, x)
    d = (out - x).cpu()
    assert (out >= x).all() and (out.double() <= x.double() + 0.1 + 2. ** -24).all()
    assert d.std() > 0.02 and abs(d.mean().item() - 0.05) < 0.002          # U[0, 0.1): std 0.0289, 21 600 draws
    # one draw per ELEMENT: the channels of a pixel differ
    assert not torch.equal(d[:, 0], d[:, 1])


@pytest.mark.parametrize('member', [lambda: m.Transform(SaltAndPepperNoise(0.2, 0.5)), lambda: GaussianNoise(0., 0.1)],
                         ids=['salt_pepper', 'uniform'])
def test_same_counter_and_seed_give_the_same_bits(member):
    x = _noise_input()
    mod = T.RandomChoice([member()]).reseed(33)
    first = _native(mod, x)
    second = _native(mod, x)
    assert mod.counter_state() == (2, 0)
    assert not torch.equal(first, second), 'the next call draws afresh'
    mod.set_counter(0)
    assert torch.equal(_native(mod, x), first)
    assert torch.equal(_native(mod, x), second)
    other = T.RandomChoice([member()]).reseed(33, instance_id=mod.instance_id + 1)
    assert not torch.equal(_native(other, x), first), 'another instance is another stream'
    again = T.RandomChoice([member()]).reseed(33, instance_id=mod.instance_id)
    assert torch.equal(_native(again, x), first)


# ---------------------------------------------------------------------------------------------- random choice
def _choice(seed, force_module_code=False):
    """salt and pepper | uniform noise | blur with a drawn sigma | crop(5) -> resize(9), for a 9 x 9 frame"""
    members = [m.Transform(SaltAndPepperNoise(0.2, 0.5)), m.Transform(GaussianNoise(0., 0.1)),
               m.Transform(T.GaussianBlur(3, sigma=(0.5, 2.0))), T.Compose([T.RandomCrop(5), T.Resize((9, 9))])]
    choice = T.RandomChoice(members).reseed(seed, instance_id=77)
    if force_module_code:
        choice._launch = lambda ops, x: None        # the pick becomes torchvision's: a host draw
    return choice


def _check_member(out, x, member, top=None, left=None, sigma=None):
    """`out` is what the module code of `member` makes of `x` with these parameters (noise members: their arithmetic)"""
    x64, o64 = x.double().cpu().numpy(), out.double().cpu().numpy()
    diff = o64 - x64
    if member == 0:
        assert np.isin(np.round(diff / 0.2), (-1, 0, 1)).all() and (np.abs(np.abs(diff[diff != 0]) - 0.2) <= 2. ** -23).all()
        assert (diff != 0).any() and np.array_equal(diff[:, 0] != 0, diff[:, 1] != 0)
    elif member == 1:
        assert (diff >= 0).all() and (diff <= 0.1 + 2. ** -24).all() and diff.std() > 0
    elif member == 2:
        assert np.abs(o64 - ref.blur(x64, 3, 3, sigma)).max() <= CEILING['blur']
    else:
        assert np.abs(o64 - ref.resize(x64[..., top:top + 5, left:left + 5], 9, 9)).max() <= CEILING['resize']


def _which_member(out, x, blur, crop):
    """which member made `out` of `x`, for a pick nothing reports (the module-code choice): tried in turn"""
    for member in range(4):
        try:
            kw = {}
            if member == 2:
                kw = dict(sigma=blur.drawn()['sigma'])
            if member == 3:
                kw = {k: crop.drawn()[k] for k in ('top', 'left')}
            _check_member(out, x, member, **kw)
            return member
        except (AssertionError, RuntimeError):
            continue
    raise AssertionError('no member explains the output')


def test_random_choice_eager():
    x = _img(1, 3, 9, 9, seed=8, lo=0.3, hi=0.7)
    choice = _choice(seed=1234)
    ops = T._native_ops(choice)
    assert [o.kind for o in ops] == ['SALT_PEPPER', 'UNIFORM_NOISE', 'BLUR', 'CROP_RESIZE']
    counts, offsets = [0, 0, 0, 0], set()
    with native.LaunchProfiler(repeat=1) as prof:
        for call in range(400):
            out = choice(x)
            d = choice.drawn()
            assert d['counter'] == call, 'the counter advances by one per call'
            counts[d['choice']] += 1
            if d['choice'] == 3:
                offsets.add((d['top'], d['left']))
            _check_member(out, x, d['choice'], d['top'], d['left'], d['sigma'])
    seen = prof.summary()
    assert list(seen) == ['asac_image_augment'] and seen['asac_image_augment']['calls'] == 400
    assert all(abs(c - 100) <= 45 for c in counts), counts                  # 5 sigma
    assert len(offsets) >= 13, 'crop offsets: at least half of the 25 valid values'
    assert all(0 <= t <= 4 and 0 <= l <= 4 for t, l in offsets)
    assert choice.counter_state() == (400, 0), 'counter, and the arrival word left at zero'


def test_random_choice_inside_a_captured_step():
    from algorithm.captured_step import CapturedStep
    x = _img(1, 3, 9, 9, seed=8, lo=0.3, hi=0.7)

    def capture(choice):
        for member in choice.transforms:        # every launcher owns its counter before the capture
            member(x)
        choice(x)
        out = torch.empty_like(x)
        step = CapturedStep.capture(lambda: out.copy_(choice(x)), DEV)
        return step, out

    # seed 1234: all four members and 11 offsets within 64 replays (fixed: the stream is a function of seed and counter)
    choice = _choice(seed=1234)
    step, out = capture(choice)
    choice.set_counter(0)
    record = []
    host_calls = []

    class Spy:
        def bracket(self, name, fn, *a, **k):
            host_calls.append(name)
            return fn(*a, **k)

    native.set_profiler(Spy())
    try:
        for replay in range(64):
            step.replay()
            d = choice.drawn()
            assert d['counter'] == replay
            _check_member(out, x, d['choice'], d['top'], d['left'], d['sigma'])
            record.append((d['choice'], d['top'], d['left'], d['sigma']))
    finally:
        native.set_profiler(None)
    assert not [c for c in host_calls if c.startswith('asac_image_')], 'a replay launches from the graph, not from the host'
    assert {r[0] for r in record} == {0, 1, 2, 3}
    assert len({r[1:3] for r in record if r[0] == 3}) >= 8
    assert choice.counter_state() == (64, 0)
    # deterministic: the eager calls from the same counter draw the same sequence
    choice.set_counter(0)
    for want in record:
        choice(x)
        d = choice.drawn()
        got = (d['choice'], d['top'], d['left'], d['sigma'])
        assert got[:3] == want[:3] and (got[3] == want[3] or (math.isnan(got[3]) and math.isnan(want[3])))

    # the defect the device draws remove: torchvision's pick is a host value, baked into the graph at capture
    torch.manual_seed(0)
    frozen = _choice(seed=1234, force_module_code=True)
    step, out = capture(frozen)
    blur, crop = frozen.transforms[2].transform, frozen.transforms[3]
    picks = []
    for _ in range(64):
        step.replay()
        picks.append(_which_member(out, x, blur, crop))
    assert len(set(picks)) == 1, 'the module-code choice replays ONE member'


# ---------------------------------------------------------------------------------------------- in the learner
def _learner(siamese, hip_config=None):
    from algorithm.utils.enums import convert_config_to_enum
    from tests.plugins import nn_views
    SAC_Base = pu.hooked_learner()

    class Recording(SAC_Base):
        siamese_losses = None

        def _train_siamese_representation_learning(self, *a, **k):
            out = super()._train_siamese_representation_learning(*a, **k)
            if not torch.cuda.is_current_stream_capturing() and self.siamese_losses is not None:
                self.siamese_losses.append(out[0].detach().clone())
            return out

    cfg = dict(siamese=siamese)
    convert_config_to_enum(cfg)
    torch.manual_seed(0)
    kw = {} if hip_config is None else {'hip_config': hip_config}
    agent = Recording(['vector', 'camera', 'segmentation'], [(6,), (3, 30, 30), (3, 30, 30)], [], 2, None, nn_views,
                      device='cuda:0', batch_size=8, n_step=3, replay_config={'capacity': 256}, **cfg, **kw)
    rng = np.random.default_rng(0)
    # (the siamese losses weigh a row by its padding mask, as the reference's do: short episodes put padded rows into every batch)
    for length in (40, 30, 50, 7, 8, 9, 7, 8, 9):
        ep = pu.synthetic_episode(rng, [(6,), (3, 30, 30), (3, 30, 30)], [], 2, (0,), length)
        ep['ep_obses_list'][1:] = [rng.random(o.shape, dtype=np.float32) for o in ep['ep_obses_list'][1:]]   # frames in [0, 1]
        agent.put_episode(**ep)
    return agent


def _choices(agent):
    return [getattr(rep, name) for rep in (agent.model_rep, agent.model_target_rep)
            for name in ('camera_transformers', 'segmentation_transformers')]


def _reseat(agent, seed):
    for i, choice in enumerate(_choices(agent)):
        choice.reseed(seed, counter=0, instance_id=500 + i)


def _record_views(agent):
    """-> a list that receives the encoders `get_augmented_encoders` returns, online then target"""
    views = []
    for rep in (agent.model_rep, agent.model_target_rep):
        def recording(obs_list, inner=rep.get_augmented_encoders):
            enc = inner(obs_list)
            views.extend(e.detach().clone() for e in enc)
            return enc
        rep.get_augmented_encoders = recording
    return views


def test_learner_on_the_views_plugin_atc():
    agent = _learner('ATC')
    picks = []
    for _ in range(12):
        agent.train()
        picks.append(agent.model_rep.camera_transformers.drawn()['choice'])
    assert agent._graph is not None, 'the step was captured'
    assert torch.isfinite(agent._params.flat).all() and math.isfinite(agent._stats['loss_q'].item())
    assert len(set(picks)) > 1, picks
    counter, arrival = agent.model_rep.camera_transformers.counter_state()
    assert counter >= 12 and arrival == 0
    agent.close()


def test_learner_on_the_views_plugin_byol_stays_finite():
    agent = _learner('BYOL')
    for _ in range(12):
        agent.train()
    assert torch.isfinite(agent._params.flat).all() and math.isfinite(agent._stats['loss_q'].item())
    agent.close()


def test_first_eager_step_equals_the_module_code_with_the_draws_forced():
    """`use_graph=False`: the launches' first step against the same step with every `RandomChoice` replaced by the module
    code of the member and offsets the launch drew.  The seed is the first whose four first draws (two images, online and
    target) are blur or crop -> resize: the per-pixel draws of the two noise members have no host counterpart to force.
    The two steps differ by the blur's and the resize's float32 rounding only (<= 5e-5 on inputs of size 1, CEILING):
    the losses and the encoders of the views agree to 1e-3 relative.  (The siamese loss weighs a row by its padding mask,
    as the reference's does, and is exactly zero for a batch without padded rows: the encoders are what always tells.)"""
    probe = _img(1, 3, 30, 30, seed=9)
    agent = _learner('ATC', {'use_graph': False})
    seed = None
    for cand in range(400):
        _reseat(agent, cand)
        firsts = []
        for choice in _choices(agent):
            choice(probe)
            firsts.append(choice.drawn()['choice'])
        if all(f in (2, 3) for f in firsts):
            seed = cand
            break
    assert seed is not None
    _reseat(agent, seed)
    agent.siamese_losses = []
    views_native = _record_views(agent)
    agent.train()
    drawn = [c.drawn() for c in _choices(agent)]
    assert [d['counter'] for d in drawn] == [0, 0, 0, 0] and [d['choice'] for d in drawn] == firsts
    loss_native, q_native = agent.siamese_losses[0].item(), agent._stats['loss_q'].item()
    agent.close()

    forced = _learner('ATC', {'use_graph': False})
    for choice, d in zip(_choices(forced), drawn):
        if d['choice'] == 2:
            choice.forward = lambda x: T.gaussian_blur(x, (9, 9), 9.)
        else:
            choice.forward = lambda x, d=d: T.resize(T.crop(x, d['top'], d['left'], 18, 18), (30, 30))
    forced.siamese_losses = []
    views_forced = _record_views(forced)
    forced.train()
    loss_forced, q_forced = forced.siamese_losses[0].item(), forced._stats['loss_q'].item()
    forced.close()
    print(f'siamese loss: launches {loss_native!r}, module code {loss_forced!r}; loss_q {q_native!r} / {q_forced!r}')
    assert math.isfinite(loss_native) and abs(loss_native - loss_forced) <= 1e-3 * abs(loss_forced)
    assert len(views_native) == len(views_forced) == 4          # two images, online and target
    for a, b in zip(views_native, views_forced):
        assert a.shape == b.shape and float(b.abs().max()) > 0
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
    assert abs(q_native - q_forced) <= 1e-3 * abs(q_forced)
