"""The host model of the segment rollout's bookkeeping (tests/segments_ref.py) against the same steps cut from one
long whole-episode simulation, on all five environments, and the C-ABI's new surface (no GPU needed).

For a scripted action sequence, K consecutive segment calls of H steps must give exactly the K*H steps of the
whole-episode simulation: the same states and rewards row by row, step_index = the step's index in its episode,
starts at every episode's first step and at every call's row 0, fragments that tile the rows and end where an episode
or the call ends with the kind of that end, t0 and episode_returns that count the episode's earlier segments in, the
carry, and the draws (action draw k of a call is the simulation's step j*H + k; the call's reset i is the
simulation's reset number (resets before the call) + i).  Everything is exact: both sides run the same float64 steps.
"""
import ctypes

import numpy as np
import pytest

import segments_ref as S

NEW_SYMBOLS = ("trpo_rollout_env_segment", "trpo_rollout_gaussian_segment", "trpo_rollout_segment_fetch",
               "trpo_rollout_carry_get", "trpo_rollout_carry_set", "trpo_rollout_carry_clear")


def scripted(name, env, n, rng):
    if name in S.cont_envs_ref.ENVS:
        return rng.uniform(-2.5, 2.5, (n, env.act_dim)).astype(np.float32)
    return rng.randint(0, env.n_actions, n)


def check_cut(name, H, ep_max, actions, K, reset_u):
    """K segments of H against run_episodes over K*H steps; returns the kinds seen"""
    env, step, reset, _ = S.env_fns(name)
    whole = S.run_episodes(step, reset, K * H, ep_max, actions, reset_u)
    carry, resets_before, kinds = None, 0, []
    for j in range(K):
        lo = j * H
        seg = S.run_segment(step, reset, carry, H, ep_max, actions[lo:lo + H], reset_u[resets_before:])
        sl = slice(lo, lo + H)
        assert np.array_equal(seg["state"], whole["state"][sl])
        assert np.array_equal(seg["reward"], whole["reward"][sl])
        assert np.array_equal(seg["step_index"], whole["t"][sl])
        want_starts = whole["starts"][sl].copy()
        want_starts[0] = 1
        assert np.array_equal(seg["starts"], want_starts)
        assert np.array_equal(seg["action_draw"], np.arange(H))          # per call: the simulation's lo + k
        # fragments: end where an episode or the call ends, tile the rows
        ends = [k for k in range(H) if whole["ended"][lo + k] or k == H - 1]
        assert list(seg["end_row"]) == ends
        assert int(seg["rows"].sum()) == H
        first = np.r_[0, seg["end_row"][:-1] + 1]
        assert np.array_equal(seg["rows"], seg["end_row"] - first + 1)
        assert np.array_equal(seg["t0"], whole["t"][lo + first])
        want_kind = [{1: S.KIND_TERMINATED, 2: S.KIND_LIMIT, 0: S.KIND_SEGMENT}[int(whole["ended"][lo + k])]
                     for k in ends]
        assert list(seg["kind"]) == want_kind
        assert list(seg["truncated"]) == [0 if k == S.KIND_TERMINATED else 1 for k in want_kind]
        assert np.array_equal(seg["episode_return"], whole["ret"][lo + np.asarray(ends)])
        assert np.array_equal(seg["final_state"], whole["next_state"][lo + np.asarray(ends)])
        # resets: one per ended episode, plus the initial one of a call that does not resume
        n_ended = int((whole["ended"][sl] != 0).sum())
        assert seg["resets"] == n_ended + (1 if carry is None else 0)
        resets_before += seg["resets"]
        assert resets_before == int(whole["episode"][lo + H - 1]) + 1 + (1 if whole["ended"][lo + H - 1] else 0)
        # the carry: the next step's state, episode step count and return so far
        s, t, ret = seg["carry"]
        last = lo + H - 1
        if whole["ended"][last]:
            assert (t, ret) == (0, 0.0) and s == list(reset(reset_u[resets_before - 1]))
        else:
            assert t == whole["t"][last] + 1 and ret == whole["ret"][last] and s == list(whole["next_state"][last])
        assert 0 <= t < ep_max
        carry = seg["carry"]
        kinds += want_kind
    return kinds


@pytest.mark.parametrize("ep_max", (3, 8))
@pytest.mark.parametrize("H", (1, 4, 17))
@pytest.mark.parametrize("name", S.ALL_ENVS)
def test_segments_cut_from_whole_episodes(name, H, ep_max):
    env = S.env_fns(name)[0]
    rng = np.random.RandomState(1000 * H + ep_max)
    K = max(4, -(-40 // H))
    actions = scripted(name, env, K * H, rng)
    reset_u = rng.uniform(size=(K * H + 2, env.reset_draws))
    kinds = check_cut(name, H, ep_max, actions, K, reset_u)
    assert S.KIND_LIMIT in kinds
    if H % ep_max:                     # the two limits are not aligned: some fragment is cut by the call
        assert S.KIND_SEGMENT in kinds


def test_terminations_inside_and_on_the_boundary():
    """CartPole-v0 pushed one way falls over after a few steps: kind 0 inside calls and, with H = 1, on every call's
    last row"""
    env = S.env_fns("CartPole-v0")[0]
    rng = np.random.RandomState(3)
    for H in (1, 4):
        K = 60 // H
        kinds = check_cut("CartPole-v0", H, 200, np.ones(K * H, np.int64), K, rng.uniform(size=(K * H + 2, 4)))
        assert S.KIND_TERMINATED in kinds and S.KIND_SEGMENT in kinds and S.KIND_LIMIT not in kinds


def test_exports_and_feed_view():
    """the built library exports the six new entry points, _lib declares them, and trpo_feed_view grew by the
    trailing step_index pointer"""
    from trpo_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert _lib.FeedView._fields_[-1][0] == "step_index"
    before = [f for f in _lib.FeedView._fields_ if f[0] != "step_index"]
    old = type("OldFeedView", (ctypes.Structure,), {"_fields_": before})
    assert ctypes.sizeof(_lib.FeedView) == ctypes.sizeof(old) + ctypes.sizeof(ctypes.c_void_p) == 88
    # resume takes its place between the parameters and the outputs
    assert _lib.SIGNATURES["trpo_rollout_env_segment"][1][3] is ctypes.c_int
