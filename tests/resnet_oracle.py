"""Plain torch restatement of ResNet-152 up to res5c as deployed in Caffe (He et al.), the yardstick of
tests/test_resnet_host.py and tests/test_gpu_resnet.py.  It works from the RAW weights -- convolution, then
batch-norm in inference form (eps 1e-5), then the scale layer -- with F.conv2d, F.batch_norm and
F.max_pool2d(ceil_mode=True), in whatever dtype it is asked for (fp64 is the truth, fp32 the error yardstick).
It shares no code with n2nmn_amd/resnet.py: names, shapes and the wiring are written out again here.

    conv1 7x7/2 pad 3 + BN + ReLU;  pool1 max 3x3/2 pad 0 ceil mode
    stages res2..res5 of bottleneck blocks, widths base * (1, 2, 4, 8), outputs 4 x the width
    block: 2a 1x1 (+BN+ReLU), 2b 3x3 pad 1 (+BN+ReLU), 2c 1x1 (+BN); out = relu(2c + shortcut)
    first block of a stage: shortcut = branch1 1x1 (+BN); stride 2 on 2a and branch1 in res3, res4, res5

Returned activations are NHWC numpy arrays keyed by Caffe's layer names; '<block>_branch2c' holds the BLOCK output
relu(branch2c + shortcut), which is what the device's fused epilogue leaves under that name.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
MEAN = (123.68, 116.779, 103.939)


def blocks_of(counts):
    out = []
    for stage, n in zip((2, 3, 4, 5), counts):
        if n <= 3:
            out.append(['res%d%s' % (stage, 'abc'[j]) for j in range(n)])
        else:
            out.append(['res%da' % stage] + ['res%db%d' % (stage, j) for j in range(1, n)])
    return out


def _bn_scale(conv):
    tail = '_conv1' if conv == 'conv1' else conv[len('res'):]
    return 'bn' + tail, 'scale' + tail


def conv_bn(x, raw, conv, stride, pad, relu, dt):
    """x NCHW -> NCHW: conv (HWIO weights) + BN + scale (+ ReLU), unfolded"""
    t = lambda k: torch.as_tensor(np.asarray(raw[k])).to(dt)
    w = t(conv + '/weights').permute(3, 2, 0, 1)
    bias = t(conv + '/biases') if conv + '/biases' in raw else None
    y = F.conv2d(x, w, bias, stride=stride, padding=pad)
    bn, sc = _bn_scale(conv)
    y = F.batch_norm(y, t(bn + '/mean'), t(bn + '/variance'), t(sc + '/gamma'), t(sc + '/beta'), False, 0.0, EPS)
    return F.relu(y) if relu else y


def pool1(x):
    return F.max_pool2d(x, kernel_size=3, stride=2, padding=0, ceil_mode=True)


def forward(images, raw, counts=(3, 8, 36, 3), dt=torch.float64, mean=MEAN):
    """images [N, H, W, 3] raw pixel values -> {layer name: NHWC numpy in dt}"""
    acts = {}

    def keep(name, y):
        acts[name] = y.permute(0, 2, 3, 1).contiguous().numpy()
        return y

    m = torch.as_tensor(np.asarray(mean, np.float32)).to(dt)          # the float32 values the device subtracts
    x = (torch.as_tensor(np.asarray(images)).to(dt) - m).permute(0, 3, 1, 2)
    x = keep('conv1', conv_bn(x, raw, 'conv1', 2, 3, True, dt))
    x = keep('pool1', pool1(x))
    for si, stage in enumerate(blocks_of(counts)):
        for j, b in enumerate(stage):
            stride = 2 if (j == 0 and si > 0) else 1
            short = keep(b + '_branch1', conv_bn(x, raw, b + '_branch1', stride, 0, False, dt)) if j == 0 else x
            y = keep(b + '_branch2a', conv_bn(x, raw, b + '_branch2a', stride, 0, True, dt))
            y = keep(b + '_branch2b', conv_bn(y, raw, b + '_branch2b', 1, 1, True, dt))
            y = conv_bn(y, raw, b + '_branch2c', 1, 0, False, dt)
            x = keep(b + '_branch2c', F.relu(y + short))
    return acts


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())
