"""prior.dense_attention (CPU): a factorized attention-weight tensor scattered into the dense (N, H, T, T) map,
against a direct element-by-element fp64 construction, for the three layer types at (l, nb) = (4, 3) and (1, 2)."""
import pytest
import torch

from prior import dense_attention


def _direct(w, mode, l, nb, N, H):
    T = l * nb
    out = torch.zeros(N, H, T, T, dtype=torch.float64)
    for n in range(N):
        for h in range(H):
            for b in range(nb):
                for i in range(l):
                    if mode == 1:
                        for bb in range(nb):
                            out[n, h, b * l + i, bb * l + i] = w[n * l + i, h, b, bb]
                    else:
                        kb = b if mode == 0 else b - 1
                        if kb < 0:
                            continue  # the zero block is no position of the sequence
                        for j in range(l):
                            out[n, h, b * l + i, kb * l + j] = w[n * nb + b, h, i, j]
    return out


@pytest.mark.parametrize("l,nb", [(4, 3), (1, 2)])
@pytest.mark.parametrize("mode,name", [(0, "row"), (1, "col"), (2, "prev row")])
def test_dense_attention_matches_direct_construction(mode, name, l, nb):
    N, H = 2, 3
    g = torch.Generator().manual_seed(10 * mode + l)
    shape = (N * l, H, nb, nb) if mode == 1 else (N * nb, H, l, l)
    w = torch.rand(shape, generator=g, dtype=torch.float64)
    if mode != 2:
        w = torch.tril(w)  # the kernels write zeros above the diagonal
    want = _direct(w, mode, l, nb, N, H)
    for key in (mode, name):
        got = dense_attention(w, key, l, N)
        assert got.shape == (N, H, l * nb, l * nb) and got.dtype == torch.float64
        assert torch.equal(got, want)
    # nothing lands on a future position, and fp32 weights stay fp32
    T = l * nb
    future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    assert not bool(want[..., future].any())
    assert dense_attention(w.float(), mode, l, N).dtype == torch.float32


def test_dense_attention_rejects_mismatched_shapes():
    with pytest.raises(ValueError):
        dense_attention(torch.zeros(6, 1, 4, 4), "diagonal", 4, 2)
    with pytest.raises(ValueError):
        dense_attention(torch.zeros(6, 1, 4, 4), 0, 5, 2)       # block length
    with pytest.raises(ValueError):
        dense_attention(torch.zeros(7, 1, 4, 4), 0, 4, 2)       # 7 items for 2 samples
    with pytest.raises(ValueError):
        dense_attention(torch.zeros(6, 1, 3, 3), 1, 4, 2)       # column layout needs N*l items
