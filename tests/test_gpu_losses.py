"""Reconstruction loss kernel (vqa_mse_loss: vqvae.py:301-307 _reconstruction_loss = mean((x - r)^2) and its
gradient 2(r - x)/n, plus an optional gradient to add) vs an fp64 restatement. The float4 kernel serves n % 4 == 0
on 16-byte aligned buffers, the scalar kernel everything else; the gradient is bitwise the same either way (the
same fp32 operations per element) and bitwise the fp32-order restatement of tests/vqvae_parity_ref.py, the loss within
fp32 summation-order rounding (1e-6 relative).

One trip of either kernel covers 1024 workgroups x 256 threads: 262,144 floats of the scalar kernel, two float4 per
thread (2,097,152 floats) of the float4 one. The sizes past 262,144 run what the smaller ones cannot: the scalar
kernel's second trip (262144 + 3), threads with a real second float4 beside threads whose second one is the clamped
repeat (4 (262144 + 1000)), and the float4 kernel's second trip (4 (524288 + 300)).
Worst observed err / bound of the loss (MI355X, profiles/vqvae_kernel_parity.txt): 0.10.
"""
import pytest
import torch

import vqa_lib as V
import vqvae_parity_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [2 * 65536, 4096 + 4, 1001, 3, 262144 + 3, 4 * (262144 + 1000), 4 * (524288 + 300)])
@pytest.mark.parametrize("with_extra", [False, True])
def test_mse_loss_forms(cuda, n, with_extra):
    g = torch.Generator().manual_seed(n)
    x, r, e = (torch.randn(n, generator=g) for _ in range(3))
    res = []
    for off in (0, 1):  # off = 1: buffers one float past a 16-byte boundary (the scalar kernel)
        def place(t):
            buf = torch.zeros(n + 8, device=cuda)
            v = buf[off:off + n]
            v.copy_(t.to(cuda))
            return v
        xd, rd, ed = place(x), place(r), place(e)
        gbuf, dr = R.guarded((n,), torch.float32, cuda, shift=off)
        loss = torch.empty(1, device=cuda)
        V.mse_loss(xd, rd, ed if with_extra else None, dr, loss)
        torch.cuda.synchronize()
        assert R.guards_intact(gbuf, dr)
        res.append((float(loss), dr.cpu()))
    want = float(((r.double() - x.double()) ** 2).mean())
    e32 = abs(float(((r - x) ** 2).mean()) - want) / want
    gref = (2.0 / n) * (r.double() - x.double()) + (e.double() if with_extra else 0.0)
    g32 = R.mse_grad(x, r, e if with_extra else None)
    for off, (lo, dr) in enumerate(res):
        R.record("mse_loss", f"n{n} extra{int(with_extra)} off{off}", e32, 1e-6, abs(lo - want) / want)
        assert abs(lo - want) <= 1e-6 * want
        assert torch.allclose(dr.double(), gref, rtol=1e-6, atol=1e-9)
        assert torch.equal(dr, g32)
    assert torch.equal(res[0][1], res[1][1])
