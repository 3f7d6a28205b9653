"""CPU: the ray encoder's one-launch convolution stack (`asac_conv1_*`, csrc/conv1d.hip) answers what it supports without a
device, its binding matches the header, and whatever the kernels do not take keeps the module path."""
import ctypes

import pytest
import torch
from torch import nn

SYMBOLS = ['asac_conv1_supported', 'asac_conv1_param_count', 'asac_conv1_backward_workspace', 'asac_conv1_backward_slabs',
           'asac_conv1_forward', 'asac_conv1_backward']

# (L, C, out1, k1, s1, out2, k2, s2): the shapes tests/test_fused_conv1d_gpu.py runs
SUPPORTED = [(400, 2, 16, 8, 4, 32, 4, 2), (61, 2, 16, 8, 4, 32, 4, 2), (67, 3, 12, 4, 2, 20, 4, 3),
             (802, 2, 16, 8, 4, 32, 4, 2), (64, 1, 16, 8, 4, 32, 4, 2), (100, 2, 16, 8, 4, 32, 3, 1)]


def test_library_exports_the_entry_points_and_the_struct_size():
    from asac_amd import native
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for name in SYMBOLS + ['asac_struct_size']:
        assert hasattr(lib, name), name
    assert native.load().asac_struct_size(b'asac_conv1_desc_t') == ctypes.sizeof(native.Conv1Desc) == 36


def test_binding_lists_the_header_argument_counts():
    from asac_amd import abi, native
    for name in SYMBOLS:
        assert name in abi.functions, f'{name} is not declared'
        params = abi.functions[name][1]
        assert name in native._SIGNATURES and len(native._SIGNATURES[name][1]) == len(params), name
    for wrapper in ('conv1_desc', 'conv1_supported', 'conv1_param_count', 'conv1_backward_workspace', 'conv1_backward_slabs',
                    'conv1_forward', 'conv1_backward'):
        assert callable(getattr(native, wrapper)), wrapper
    assert native.ABI_VERSION == 91, 'pure additions: the ABI version stays'


@pytest.mark.parametrize('shape', SUPPORTED)
def test_supported_shapes(shape):
    from asac_amd import native
    desc = native.conv1_desc(*shape, 0.01)
    assert native.conv1_supported(desc)
    L, C, o1, k1, s1, o2, k2, s2 = shape
    assert native.conv1_param_count(desc) == o1 * C * k1 + o1 + o2 * o1 * k2 + o2
    # one slab per workgroup, a number that depends on N and the descriptor only
    slabs = native.conv1_backward_slabs(desc, 37)
    assert 1 <= slabs <= 37 and native.conv1_backward_workspace(desc, 37) == slabs * native.conv1_param_count(desc)
    assert native.conv1_backward_slabs(desc, 1) == 1
    assert native.conv1_backward_slabs(desc, 1 << 20) == native.conv1_backward_slabs(desc, 1 << 21)   # (capped)


def test_default_stack_parameter_count():
    from asac_amd import native
    assert native.conv1_param_count(native.conv1_desc(400, 2, 16, 8, 4, 32, 4, 2, 0.01)) == 2352


@pytest.mark.parametrize('shape,slope,why', [
    ((64, 1, 16, 3, 1, 32, 4, 2), 0.01, 'C k1 = 3 is not a multiple of 4'),
    ((400, 2, 17, 8, 4, 32, 4, 2), 0.01, 'out1 = 17'),
    ((400, 2, 16, 8, 4, 33, 4, 2), 0.01, 'out2 = 33'),
    ((400, 2, 16, 8, 4, 32, 4, 2), 0.0, 'slope 0: the sign of y would not be the sign of z2'),
    ((400, 2, 16, 8, 4, 32, 4, 2), -0.1, 'negative slope'),
    ((400, 2, 16, 8, 4, 32, 4, 2), float('inf'), 'slope not finite'),
    ((400, 2, 16, 8, 4, 32, 4, 2), float('nan'), 'slope not finite'),
    ((19, 2, 16, 8, 4, 32, 4, 2), 0.01, 'L1 = 3 < k2: no output position'),
    ((7, 2, 16, 8, 4, 32, 4, 2), 0.01, 'L < k1'),
    ((400, 2, 16, 8, 4, 32, 20, 2), 0.01, 'out1 k2 = 320 > 256'),
    ((400, 10, 16, 8, 4, 32, 4, 2), 0.01, 'C k1 = 80 > 64'),
])
def test_unsupported_shapes(shape, slope, why):
    from asac_amd import native
    desc = native.conv1_desc(*shape, slope)
    assert not native.conv1_supported(desc), why
    assert native.conv1_param_count(desc) == -1 and native.conv1_backward_slabs(desc, 8) == -1


def _stack(C=2, pad=0, act2=None):
    return nn.Sequential(nn.Conv1d(C, 16, 8, 4, padding=pad), nn.LeakyReLU(), nn.Conv1d(16, 32, 4, 2),
                         act2 if act2 is not None else nn.LeakyReLU())


class _CudaLike:
    """a stand-in that claims to be a device tensor, for the checks `conv1d_stack_desc` makes in front of the library's answer"""

    def __init__(self, *shape):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = torch.Size(shape), True, torch.float32, False

    def dim(self):
        return len(self.shape)


def test_stack_desc_refuses_what_the_kernels_do_not_take():
    from algorithm.fused_conv import conv1d_stack_desc
    assert conv1d_stack_desc(_stack(), torch.randn(3, 400, 2)) is None, 'a CPU tensor'
    x = _CudaLike(3, 400, 2)
    desc = conv1d_stack_desc(_stack(), x)
    assert desc is not None and (desc.length, desc.channels, desc.out2) == (400, 2, 32)
    assert abs(desc.negative_slope - 0.01) < 1e-9
    assert conv1d_stack_desc(_stack(act2=nn.ReLU()), x) is None, 'another activation'
    relu_first = nn.Sequential(nn.Conv1d(2, 16, 8, 4), nn.ReLU(), nn.Conv1d(16, 32, 4, 2), nn.ReLU())
    assert conv1d_stack_desc(relu_first, x) is None
    assert conv1d_stack_desc(_stack(pad=1), x) is None, 'padding'
    assert conv1d_stack_desc(_stack(act2=nn.LeakyReLU(0.2)), x) is None, 'unequal slopes'
    assert conv1d_stack_desc(_stack(C=3), x) is None, 'channel counts'
    assert conv1d_stack_desc(list(_stack()), x) is None, 'not a Sequential'


def test_cpu_rays_take_the_module_path_whatever_the_switch():
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import image_layers
    torch.manual_seed(0)
    layer = m.Conv1dLayers(61, 2, 'default', out_dense_n=64, out_dense_depth=2)
    x = torch.randn(3, 5, 61, 2)
    assert image_layers.FUSED_CONV1D in (True, False)
    before = image_layers.FUSED_CONV1D
    try:
        outs = []
        for flag in (True, False):
            image_layers.FUSED_CONV1D = flag
            outs.append(layer(x))
    finally:
        image_layers.FUSED_CONV1D = before
    assert outs[0].shape == (3, 5, 64) and torch.equal(outs[0], outs[1])
