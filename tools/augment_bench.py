"""What an image augmentation costs as ONE launch (`asac_image_augment`, csrc/image.hip) and as the module code of the same
transform (`algorithm/utils/image_transforms.py` with its launch switched off: reflect-pad copy + depthwise conv2d,
interpolate, rand + where chains, host draws), in one process on one box and commit.

Frames: 768 (usv_search's batch 256 x n-step 3) of 84 x 84 x 3 and of 30 x 30 x 3.  Rows: each op alone and the four-member
`RandomChoice` of the views plugin.  Two modes: `eager` (microseconds a call from the host, every timed window ends in a
device synchronise) and `captured` (the call inside a `CapturedStep`, microseconds a replay).  The two ways alternate
(module, launch, module, launch, ...); the median of the rounds is reported, all rounds are listed.  One JSON line per row.

`--warp`: the rows of `asac_image_warp` instead — `RandomResizedCrop` and `ElasticTransform(100, 5)` with NEAREST and the
two-member `RandomChoice` of ugv_parking, plus the elastic transform on ONE plane: what building the field costs a call (every
workgroup builds it, so the rest of the full row is the planes).  The module code of the elastic transform copies its host
noise to the device, which no capture takes: in `captured` mode its side of these rows stays eager (`module_mode`).

    python tools/augment_bench.py [--warp] [--calls 200] [--frames 768]"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS = 5


def transforms(size):
    import algorithm.nn_models as m
    from algorithm.utils import image_transforms as T
    from algorithm.utils.transform import GaussianNoise, SaltAndPepperNoise
    crop = 50 if size == 84 else 18

    def crop_resize():
        return T.Compose([T.RandomCrop(crop), T.Resize((size, size))])

    return {
        'blur_k9_sigma9': lambda: T.GaussianBlur(9, sigma=9),
        'blur_k9_sigma_range': lambda: T.GaussianBlur(9, sigma=(0.1, 2.0)),
        'brightness': lambda: T.ColorJitter(brightness=(1.2, 1.2)),
        'blur_then_brightness': lambda: T.Compose([T.GaussianBlur(9, sigma=9), T.ColorJitter(brightness=(1.2, 1.2))]),
        'crop_resize': crop_resize,
        'salt_pepper': lambda: T.RandomChoice([m.Transform(SaltAndPepperNoise(0.2, 0.5))]),
        'uniform_noise': lambda: T.RandomChoice([m.Transform(GaussianNoise())]),
        'choice_of_four': lambda: T.RandomChoice([m.Transform(SaltAndPepperNoise(0.2, 0.5)), m.Transform(GaussianNoise()),
                                                  m.Transform(T.GaussianBlur(9, sigma=9)), m.Transform(crop_resize())]),
    }


def warp_transforms(size):
    import algorithm.nn_models as m
    from algorithm.utils import image_transforms as T
    nearest = T.InterpolationMode.NEAREST

    def rrc():
        return T.RandomResizedCrop(size=(size, size), scale=(0.8, 0.9), interpolation=nearest)

    def elastic():
        return T.ElasticTransform(alpha=100, sigma=5, interpolation=nearest)

    return {
        'resized_crop_nearest': rrc,
        'elastic_100_5': elastic,
        'elastic_100_5_one_plane': elastic,
        'choice_of_two': lambda: T.RandomChoice([m.Transform(rrc()), m.Transform(elastic())]),
    }


def module_code(module):
    """the same transform with every launch switched off"""
    from algorithm.utils.image_transforms import _Launcher
    for sub in module.modules():
        if isinstance(sub, _Launcher):
            sub._launch = lambda ops, x: None
    return module


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def row(name, build, x, calls, mode, capture_module=True):
    from algorithm.captured_step import CapturedStep
    from asac_amd import native
    ways = {'module': module_code(build()), 'launch': build()}
    out = {'mode': mode, 'op': name, 'frames': x.shape[0], 'size': x.shape[-1], 'calls': calls, 'rounds': ROUNDS}
    fns = {}
    for tag, mod in ways.items():
        for _ in range(3):
            mod(x)
        with native.LaunchProfiler(repeat=1) as prof:
            mod(x)
        out['image_launches_' + tag] = sum(v['calls'] for k, v in prof.summary().items() if k.startswith('asac_image_'))
        if mode == 'captured' and (tag == 'launch' or capture_module):
            step = CapturedStep.capture(lambda mod=mod: mod(x), x.device)
            step.replay()
            fns[tag] = step.replay
        else:
            fns[tag] = lambda mod=mod: mod(x)
    runs = {tag: [] for tag in ways}
    for _ in range(ROUNDS):
        for tag in ways:
            runs[tag].append(round(timed(fns[tag], calls), 2))
    for tag in ways:
        out['us_' + tag] = median(runs[tag])
        out['us_' + tag + '_rounds'] = runs[tag]
    if mode == 'captured' and not capture_module:
        out['module_mode'] = 'eager'
    out['ratio'] = round(out['us_module'] / out['us_launch'], 2)
    # what one read and one write of the frames would take at 1 TB/s, for scale
    out['bytes_moved'] = 2 * x.numel() * 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--frames', type=int, default=768)
    ap.add_argument('--only', default=None, help='one op name')
    ap.add_argument('--warp', action='store_true', help='the rows of asac_image_warp')
    args = ap.parse_args()
    import asac_amd  # noqa: F401
    assert torch.cuda.is_available(), 'needs cuda:0'
    gen = torch.Generator().manual_seed(0)
    for size in (84, 30):
        x = torch.rand(args.frames, 3, size, size, generator=gen).cuda()
        for name, build in (warp_transforms if args.warp else transforms)(size).items():
            if args.only and name != args.only:
                continue
            frames = x[:1, :1] if name.endswith('_one_plane') else x
            for mode in ('eager', 'captured'):
                # (the elastic module code's host noise cannot be captured)
                print(json.dumps(row(name, build, frames, args.calls, mode, capture_module=not args.warp or 'resized' in name)),
                      flush=True)


if __name__ == '__main__':
    main()
