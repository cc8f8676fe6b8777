"""sampler.prompt_windows, the window rule of prompted long-form sampling, on the host: over a grid of small values the
windows are window_starts' with their indices, the skipped ones are exactly those that end inside the known codes,
the prime is capped at the window, and the drawn ranges tile [P, total) once."""
import pytest

from sampler import prompt_windows, window_starts

N_CTX = 8
GRID = [(total, hop, P) for hop in (1, 4, 8) for total in range(8, 41) for P in range(1, total)]


def test_grid_is_not_empty():
    assert len(GRID) == 3 * sum(total - 1 for total in range(8, 41))


@pytest.mark.parametrize("hop", [1, 4, 8])
def test_windows_over_the_grid(hop):
    skipped_somewhere = primed_full_somewhere = False
    for total, h, P in GRID:
        if h != hop:
            continue
        starts = window_starts(total, N_CTX, hop)
        got = prompt_windows(total, N_CTX, hop, P)
        drawn = []
        known = P
        ran = {w for w, _, _ in got}
        for w, start in enumerate(starts):
            if start + N_CTX <= known:     # ends at or before the known length: launches nothing
                assert w not in ran, (total, hop, P, w)
                skipped_somewhere = True
                continue
            assert w in ran, (total, hop, P, w)
            known = start + N_CTX
        known = P
        for w, start, prime_len in got:
            assert starts[w] == start, (total, hop, P, w)              # index and start are window_starts'
            assert 0 <= prime_len < N_CTX, (total, hop, P, w)          # capped at the window, something is drawn
            assert prime_len == min(known, start + N_CTX) - start, (total, hop, P, w)
            primed_full_somewhere |= prime_len == N_CTX - 1
            drawn += list(range(start + prime_len, start + N_CTX))
            known = start + N_CTX
        assert [w for w, _, _ in got] == sorted(ran)
        assert drawn == list(range(P, total)), (total, hop, P)         # [P, total), nothing twice, in order
    assert skipped_somewhere and primed_full_somewhere


@pytest.mark.parametrize("total,hop", [(8, 4), (20, 4), (33, 8), (40, 1)])
def test_no_prompt_is_every_window_with_the_overlap_as_its_prime(total, hop):
    starts = window_starts(total, N_CTX, hop)
    got = prompt_windows(total, N_CTX, hop, 0)
    assert [(w, s) for w, s, _ in got] == list(enumerate(starts))
    assert got[0][2] == 0
    for (w, s, prime_len), before in zip(got[1:], starts):
        assert prime_len == before + N_CTX - s


def test_worked_example():
    # total 20, windows of 8 every 4: starts 0 4 8 12. 13 known codes: windows 0 and 1 end at 8 and 12 and are
    # skipped, window 2 (8 .. 16) is primed with 5 codes, window 3 (12 .. 20) with the 4 it shares with window 2
    assert window_starts(20, 8, 4) == [0, 4, 8, 12]
    assert prompt_windows(20, 8, 4, 13) == [(2, 8, 5), (3, 12, 4)]
    assert prompt_windows(20, 8, 4, 12) == [(2, 8, 4), (3, 12, 4)]      # exactly on a window end
    assert prompt_windows(20, 8, 4, 16) == [(3, 12, 4)]
    assert prompt_windows(20, 8, 4, 19) == [(3, 12, 7)]
    assert prompt_windows(20, 8, 4, 1) == [(0, 0, 1), (1, 4, 4), (2, 8, 4), (3, 12, 4)]


@pytest.mark.parametrize("args", [(20, 8, 4, 20), (20, 8, 4, 25), (20, 8, 4, -1), (7, 8, 4, 1), (20, 8, 0, 1),
                                  (20, 8, 9, 1)])
def test_bad_arguments_raise(args):
    with pytest.raises(ValueError):
        prompt_windows(*args)
