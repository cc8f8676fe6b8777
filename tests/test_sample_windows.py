"""The window rule of long-form sampling (sampler.window_starts), no GPU: which windows of one level's context
cover a longer run of codes."""
import pytest

from sampler import window_starts


@pytest.mark.parametrize("total,n_ctx,hop,want", [(160, 64, 32, [0, 32, 64, 96]), (150, 64, 32, [0, 32, 64, 86]),
                                                  (64, 64, 32, [0]), (65, 64, 64, [0, 1])])
def test_window_starts(total, n_ctx, hop, want):
    got = window_starts(total, n_ctx, hop)
    assert got == want
    assert len(set(got)) == len(got) and got[-1] + n_ctx == total


@pytest.mark.parametrize("total,n_ctx,hop", [(4, 4, 2), (8, 4, 2), (32, 16, 8), (128, 64, 32), (131, 64, 1), (200, 64, 64)])
def test_windows_cover_the_length_without_gaps(total, n_ctx, hop):
    """Every window starts inside (or right at the end of) what the windows before it have covered."""
    covered = 0
    for start in window_starts(total, n_ctx, hop):
        assert 0 <= start <= covered
        covered = max(covered, start + n_ctx)
    assert covered == total


@pytest.mark.parametrize("total,n_ctx,hop", [(63, 64, 32), (128, 64, 0), (128, 64, 65)])
def test_window_starts_rejects(total, n_ctx, hop):
    with pytest.raises(ValueError):
        window_starts(total, n_ctx, hop)
