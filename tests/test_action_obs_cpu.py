"""Action rows in the fused env step's observation, without a GPU (include/roboy_sim.h: rb_env_action_obs_*): the test
helper's list-based statement of the K blocks against a ring of S slots indexed by the step counter - what csrc/env_hist.hpp keeps -,
the host-only column count, and RoboyVecEnv's space arithmetic."""
import numpy as np
import pytest

from action_obs_util import MAX_ROWS, HistoryBook, clip_action, ring_slots
from gym_roboy_amd import _native as nat


def test_ring_slot_counts():
    assert ring_slots(0, 0) == 0 and ring_slots(1, 0) == 1 and ring_slots(2, 0) == 2 and ring_slots(3, 0) == 4
    assert ring_slots(0, 3) == 4 and ring_slots(2, 3) == 4 and ring_slots(5, 3) == 8 and ring_slots(8, 7) == 8 and ring_slots(8, 0) == 8
    assert ring_slots(1, 7) == 8 and ring_slots(4, 4) == 8
    for rows in range(1, MAX_ROWS + 1):
        for hi in range(8):
            s = ring_slots(rows, hi)
            assert s & (s - 1) == 0 and s > max(hi, rows - 1) and (s == 1 or s // 2 <= max(hi, rows - 1))


def _ring_run(rows, delay_hi, auto_reset, steps, seed):
    """One env per episode length out of {1, 2, S - 1, S, S + 3} (twice: two action streams), stepped against a ring of S slots:
    every env stores the row it is handed into slot k mod S and reads block j from slot (k - j) mod S while k - j >= 1 - block 0
    from the handed row itself.  Returns [(blocks of the ring, blocks of the book)] per step."""
    S = ring_slots(rows, delay_hi)
    lengths = np.array(sorted({L for L in (1, 2, S - 1, S, S + 3) if L >= 1}) * 2, np.int64)
    n, n_t = len(lengths), 3
    rng = np.random.default_rng(seed)
    ring = rng.uniform(5, 6, (S, n, n_t)).astype(np.float32)       # (stale slots must never show: nothing here is within [-1, 1])
    k = np.ones(n, np.int64)
    book = HistoryBook(n, n_t, rows)
    out = []
    for _ in range(steps):
        act = rng.uniform(-2, 2, (n, n_t)).astype(np.float32)
        ring[k & (S - 1), np.arange(n)] = act
        done = k + 1 > lengths                                     # (env_account: sn = k + 1 > max_len)
        reset = done & auto_reset
        got = np.zeros((n, rows, n_t), np.float32)
        for j in range(rows):
            live = ~reset & (k - j >= 1)
            src = act if j == 0 else ring[(k - j) & (S - 1), np.arange(n)]
            got[live, j] = clip_action(src[live])
        out.append((got.reshape(n, -1), book.blocks(act, done, auto_reset)))
        k = np.where(reset, 1, k + 1)
        assert np.array_equal(k, book.k)
    return out, lengths


@pytest.mark.parametrize("rows", range(1, MAX_ROWS + 1))
def test_history_book_is_the_ring_indexed_by_the_counter(rows):
    for delay_hi in range(8):
        steps = 3 * (ring_slots(rows, delay_hi) + 3) + 2
        out, lengths = _ring_run(rows, delay_hi, True, steps, 100 * rows + delay_hi)
        saw_clamp = saw_zero_block = False
        for ring_blocks, book_blocks in out:
            assert np.array_equal(ring_blocks, book_blocks), (rows, delay_hi)
            assert np.abs(book_blocks).max() <= 1.0
            saw_clamp |= bool((np.abs(book_blocks) == 1.0).any())
            saw_zero_block |= bool((book_blocks.reshape(len(lengths), rows, -1) == 0).all(axis=2).any())
        assert saw_clamp and saw_zero_block


def test_history_book_without_auto_reset_runs_on():
    """counter and history run on through done: after K steps no block is zero any more, whatever the episode length"""
    rows = 4
    out, lengths = _ring_run(rows, 0, False, 12, 7)
    for ring_blocks, book_blocks in out:
        assert np.array_equal(ring_blocks, book_blocks)
    assert not (out[-1][1].reshape(len(lengths), rows, -1) == 0).all(axis=2).any()


def test_history_book_by_hand():
    book = HistoryBook(2, 1, 3)
    a = [np.array([[0.5], [-3.0]], np.float32), np.array([[2.0], [0.25]], np.float32), np.array([[-0.5], [0.75]], np.float32)]
    assert np.array_equal(book.blocks(a[0], [False, False]), [[0.5, 0, 0], [-1.0, 0, 0]])
    assert np.array_equal(book.blocks(a[1], [False, True]), [[1.0, 0.5, 0], [0, 0, 0]])          # env 1 was auto-reset: zero blocks
    assert np.array_equal(book.blocks(a[2], [False, False]), [[-0.5, 1.0, 0.5], [0.75, 0, 0]])    # ... and starts over
    assert np.array_equal(book.reset_blocks(), np.zeros((2, 3), np.float32))


def test_action_obs_count_is_the_formula_and_refuses():
    count = nat.load().rb_env_action_obs_count
    obs_count = nat.load().rb_env_obs_count
    for n_q, n_t in ((3, 8), (3, 12), (3, 1), (3, 16), (20, 38), (0, 0)):
        for mask in range(16):
            for rows in range(0, nat.RB_ACTION_OBS_MAX + 1):
                want = 3 * n_q + bin(mask).count("1") * n_t + rows * n_t
                assert count(n_q, n_t, mask, rows) == want
            assert count(n_q, n_t, mask, 0) == obs_count(n_q, n_t, mask)
    assert count(3, 8, 9, 3) == 49 and count(3, 8, 15, 8) == 105 and count(3, 12, 0, 3) == 45
    assert nat.RB_ACTION_OBS_MAX == MAX_ROWS == 8
    for bad in ((3, 8, 0, -1), (3, 8, 0, 9), (3, 8, 16, 1), (-1, 8, 0, 1), (3, -2, 0, 1), (3, 8, 1 << 31, 0)):
        assert count(*bad) == -1, bad


def test_vec_env_space_arithmetic():
    from gym_roboy_amd.envs.vec_env import action_obs_bounds, action_obs_rows
    assert action_obs_rows(None) == 0 and action_obs_rows(0) == 0 and action_obs_rows(8) == 8 and action_obs_rows(np.int64(3)) == 3
    for bad in (-1, 9, 2.0, "3", True, (1, 2)):
        with pytest.raises(ValueError):
            action_obs_rows(bad)
    low, high = np.arange(-25, 0, dtype=np.float32), np.arange(1, 26, dtype=np.float32)
    for rows in (0, 1, 3, 8):
        lo, hi = action_obs_bounds(low, high, 8, rows)
        assert lo.dtype == hi.dtype == np.float32
        assert lo.shape == hi.shape == (nat.load().rb_env_action_obs_count(3, 8, 9, rows),)
        assert np.array_equal(lo[:25], low) and np.array_equal(hi[:25], high)
        assert np.all(lo[25:] == -1.0) and np.all(hi[25:] == 1.0)
