"""Plain Adam (vqa_adam_keras, vqa_optim.hip adam_stride_kernel<false>) on its own: TF ApplyAdam over a flat fp32
buffer,
    m += (g gs - m)(1 - b1);  v += ((g gs)^2 - v)(1 - b2);  w -= (m alpha) / (sqrt(v) + eps),
    alpha = lr sqrt(1 - b2^t) / (1 - b1^t), t = step + 1 read from the device.

Sizes from one element to one past the launch cap (4096 workgroups x 256 threads = 1,048,576 elements a trip, so
1,048,576 + 259 runs the second trip), buffers cut from NaN-filled ones at a 16-byte boundary and one float past it
(the kernel is scalar: it must not care), three steps from non-zero m and v (the first-step shortcut m = (1 - b1) g
cannot hide an error), grad_scale = 0.5, the rate from the host and from a device scalar that must win over the host
value passed beside it.

m and v: bitwise the fp32-order restatement (tests/vqvae_parity_ref.py). w: within 1e-6 (|w| + 1e-2) of
oracle.vqvae_ref.keras_adam in fp64 with TF's float32 step size (adam_alpha_f32), the bound of
tests/test_gpu_schedule.py for the same update (only powf differs). g is only read.
Worst observed err / bound of w (MI355X, profiles/vqvae_kernel_parity.txt): 0.14.
"""
import numpy as np
import pytest
import torch

import vqa_lib as V
import vqvae_parity_ref as R
from oracle.vqvae_ref import adam_alpha_f32, keras_adam

pytestmark = pytest.mark.gpu
CAP = 4096 * 256


def f32(c):
    return float(np.float32(c))


@pytest.mark.parametrize("lr_on_device", [False, True], ids=["host_lr", "device_lr"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [1, 255, 4099, CAP + 259])
def test_adam_keras_three_steps(cuda, n, shift, lr_on_device):
    b1, b2, eps, gs, lr = f32(0.9), f32(0.999), f32(1e-7), 0.5, f32(3e-3)
    g = R.gen(n + shift)
    w0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g) * 1e-2 + 1e-4
    bufs = [R.guarded((n,), torch.float32, cuda, shift=shift) for _ in range(3)]
    (wb, w), (mb, m), (vb, v) = bufs
    w.copy_(w0.cuda()), m.copy_(m0.cuda()), v.copy_(v0.cuda())
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    # the device rate differs from the host value passed beside it: the device value must win
    lr_dev = torch.tensor([lr], device=cuda) if lr_on_device else None
    lr_host = 7.0 if lr_on_device else lr
    wc, mc, vc = w0, m0, v0
    worst = 0.0
    for t in (1, 2, 3):
        grad = torch.randn(n, generator=g)
        gd = grad.cuda()
        step.fill_(t - 1)
        V.adam_keras(w, gd, m, v, step, lr_host, b1, b2, eps, gs, lr_dev=lr_dev)
        torch.cuda.synchronize()
        assert all(R.guards_intact(b, t_) for b, t_ in bufs)
        assert torch.equal(gd.cpu(), grad)
        mw, vw = R.adam_mv(grad, mc, vc, b1, b2, gs)
        assert torch.equal(m.cpu(), mw) and torch.equal(v.cpu(), vw)
        ww, _, _ = keras_adam(wc.double(), grad.double() * gs, mc.double(), vc.double(), t, lr=lr, b1=b1, b2=b2,
                              eps=eps, alpha=adam_alpha_f32(lr, t))
        got = w.cpu()
        ratio = float(((got.double() - ww).abs() / (1e-6 * (ww.abs() + 1e-2))).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (t, ratio)
        wc, mc, vc = got, mw, vw   # continue from the device state: fp32 rounding does not accumulate into the check
    R.record("adam_w", f"n{n} off{shift} {'device' if lr_on_device else 'host'} lr, 3 steps", 0.0, 1.0, worst)
