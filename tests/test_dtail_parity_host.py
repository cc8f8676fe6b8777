"""CPU-only side of the decoder tail's parity suite: the launch plans tests/test_gpu_dtail.py claims, the plain fp64
restatement of tests/dtail_parity_ref.py against the two-layer oracle at 1e-12, and the sensitivity of the bounds: the
restatement damaged the way a kernel goes wrong must break the very bound the GPU test applies, at the GPU test's
shapes (a smaller batch with the same T where the batch only multiplies the work and leaves the plan's kind alone).
"""
import pytest
import torch

import dtail_parity_ref as D

F32, BF16 = torch.float32, torch.bfloat16


def test_plans_of_the_gpu_cases():
    for (B, T), want in D.FWD_CASES.items():
        assert D.fwd_plan(B, T) == want, (B, T)
    for (B, T), want in D.BWD_CASES.items():
        assert D.bwd_plan(B, T) == want, (B, T)
    # what the old direct test reached: one forward pass at its largest case, and no single stage at P >= 64
    assert D.fwd_plan(2, 70001) == (274, 1)
    assert D.bwd_plan(2, 70001)[1:3] == (512, 32) and D.bwd_plan(4, 1000)[1:3] == (32, 0)
    # the training shape: six forward passes
    assert D.fwd_plan(32, 32768) == (24, 6)
    assert D.bwd_plan(272, 300) == (1, 272, 17, 3)
    # every row of an item is in exactly one partial row
    for B, T in D.BWD_CASES:
        gx, P, _, _ = D.bwd_plan(B, T)
        seen = torch.zeros(B, T, dtype=torch.int32)
        for p in range(P):
            n, spans = D.part_rows(B, T, p)
            for a, b in spans:
                seen[n, a:b] += 1
        assert bool((seen == 1).all()), (B, T)


@pytest.mark.parametrize("B,T,Cu,bias", [(2, 70, 64, True), (3, 37, 48, True), (1, 1, 64, True), (2, 2, 33, True),
                                         (2, 300, 1, True), (2, 70, 130, True), (2, 64, 64, False), (3, 257, 65, True)])
def test_restatement_matches_the_two_layer_oracle(B, T, Cu, bias):
    h, dy = D.inputs(B, T, F32)
    w_up, b_up, w_out, b_out = D.params(Cu, T)
    if not bias:
        b_up = b_out = None
    ref = D.oracle(h, dy, w_up, b_up, w_out, b_out)
    got = D.composite(h, dy, w_up, b_up, w_out, b_out)
    for k in D.NAMES:
        assert got[k].shape == ref[k].shape, k
        assert D.rel(got[k], ref[k]) < 1e-12, (k, D.rel(got[k], ref[k]))


# (B, T) of the GPU test with the batch cut where it only multiplies the work: the forward's defects sit at a row of
# the item whatever the batch; the backward's partial rows keep their plan (272 items of 300 rows: one block per item,
# three passes, two stages, as at 512)
SENS_SHAPES = [(2, 257), (2, 512), (2, 1300), (2, 300), (4, 2048), (3, 3000), (65, 100), (272, 300), (2, 70), (2, 1)]


def _case_bounds(B, T, Cu, ref, args):
    names = D.long_sums(B, Cu)
    measured = D.fp32_oracle_error(ref, *args, names) if names else {}
    return {k: D.bound(measured.get(k)) for k in D.NAMES}


def test_bounds_see_every_planted_defect(capsys):
    """fp32 bound on every output, and the bf16 per-element bound on dh, against each defect; none may pass at every
    shape, and the undamaged restatement passes at all of them."""
    seen = {}
    for B, T in SENS_SHAPES:
        h, dy = D.inputs(B, T, F32)
        p = D.params(64, T)
        ref = D.composite(h, dy, *p)
        bounds = _case_bounds(B, T, 64, ref, (h, dy, *p))
        for name in D.DEFECTS:
            if (name == "halo row dropped at the pass boundary" and T <= D.FWD_ROWS) or \
                    (name == "halo row dropped at a wave boundary" and T <= 64) or \
                    (name.startswith("partial row") and D.bwd_plan(B, T)[1] < 2):
                continue
            bad = D.composite(h, dy, *p, defect=name)
            worst = max(D.rel(bad[k], ref[k]) / bounds[k] for k in D.NAMES)
            seen.setdefault(name, []).append(((B, T), worst))
            with capsys.disabled():
                print(f"dtail B={B} T={T} {name:40s} worst error / bound {worst:10.3g}")
    assert set(seen) == set(D.DEFECTS)
    for name, rows in seen.items():
        assert max(w for _, w in rows) > 1.0, (name, rows)
    # the defects a plan makes possible are seen at the shapes that reach the plan
    at = {name: dict(rows) for name, rows in seen.items()}
    for shape in [(2, 257), (2, 512), (2, 1300), (2, 300)]:
        assert at["halo row dropped at the pass boundary"][shape] > 1.0
    for shape in [(4, 2048), (3, 3000), (65, 100), (272, 300)]:
        assert at["partial row lost"][shape] > 1.0 and at["partial row counted twice"][shape] > 1.0
    for name in ("t = 0 edge omitted", "t = 2T - 1 edge omitted"):
        assert at[name][(2, 1)] > 1.0


def test_old_bf16_dh_bound_lets_a_small_element_through():
    """1e-2 of the tensor's max-abs passes a value that is wrong by half of itself on a small element; the
    per-element bound does not."""
    h, dy = D.inputs(2, 70, BF16)
    ref = D.composite(h.float(), dy, *D.params(64, 70))["dh"]
    bad = ref.clone()
    i = int(ref.abs().flatten().kthvalue(ref.numel() // 100).indices)     # a small element
    bad.view(-1)[i] *= 1.5
    assert D.rel(bad, ref) < 1e-2
    assert D.bf16_dh_excess(bad, ref) > 1.0


def test_bf16_rounding_of_the_reference_is_inside_the_dh_bound():
    """every bf16 case of the GPU test, at its full size (dh of the restatement: no 64-channel intermediate). bf16
    keeps 8 significant bits, so one round-to-nearest moves a value by up to 2^-8 of itself (measured here: 0.98 of the
    2^-8 |ref| term at B = 768, T = 257): the rounding alone may use the whole first term, and the second term is what
    is left for the fp32 arithmetic in front of it."""
    shapes = list(D.FWD_CASES) + list(D.BWD_CASES) + [(2, 70)]
    for B, T in shapes:
        for Cu in ((64, 130) if (B, T) == (2, 70) else (64,)):
            h, dy = D.inputs(B, T, BF16)
            w_up, b_up, w_out, b_out = D.params(Cu, T)
            dh = _dh_only(h.float(), dy, w_up, w_out)
            ex = D.bf16_dh_excess(dh.to(BF16), dh)
            assert 0.5 < ex <= 1.0, (B, T, Cu, ex)


def _dh_only(h, dy, w_up, w_out):
    """dh of the restatement without the parameter gradients (cheap at B = 1000)"""
    z = torch.zeros
    B, T, _ = h.shape
    out = []
    for n0 in range(0, B, 128):
        r = D.composite(h[n0:n0 + 128], dy[n0:n0 + 128], w_up, z(w_up.shape[1]), w_out, z(1))
        out.append(r["dh"])
    return torch.cat(out)
