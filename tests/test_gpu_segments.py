"""Fixed-horizon segment rollouts on the device (rollout_segment_kernel through the C-ABI): environments that persist
across calls, under both heads.

The steps of a segment are the whole-episode kernel's, so K segment calls of T steps are compared bit for bit with
the first K*T rows per environment of one whole-episode rollout on the same injected draws (that kernel is held to
the host references by test_gpu_envs.py and test_gpu_cont_envs.py).  The bookkeeping -- step_index, starts, kinds,
t0, episode_returns, carry -- is compared exactly with the host model tests/segments_ref.py, replaying the rewards,
terminations and states the device recorded.  Bars that are not exact are test_gpu_truncation.py's: returns rtol
1e-13, standardised advantages rtol 1e-11 / atol 1e-12.
"""
import numpy as np
import pytest

import segments_ref as S
from gae_ref import gae_ref
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

HIDDEN = [8]
GAMMA, LAM = 0.95, 0.95
ROW_KEYS = ("obs", "obs32", "actions", "head", "rewards", "draw")


def is_cont(name):
    return name in S.cont_envs_ref.ENVS


def make_engine(name, max_rows=4096, seed=11):
    from trpo_amd import Engine, xavier_theta
    env = S.env_fns(name)[0]
    cont = is_cont(name)
    A = env.act_dim if cont else env.n_actions
    e = Engine(env.obs_dim, HIDDEN, A, max_rows=max_rows, dist="gaussian" if cont else "categorical")
    th = xavier_theta(env.obs_dim, HIDDEN, A, np.random.RandomState(seed))
    if cont:
        th = np.concatenate([th, np.full(A, -0.5, np.float32)])
    e.set_flat(th)
    return e, th, env


def whole(e, name, **kw):
    draws = kw.pop("draws", None)
    if is_cont(name):
        return e.rollout_gaussian(name, action_normals=draws, **kw)
    return e.rollout(name, action_uniforms=draws, **kw)


def segment(e, name, **kw):
    draws = kw.pop("draws", None)
    if is_cont(name):
        return e.rollout_gaussian_segment(name, action_normals=draws, **kw)
    return e.rollout_segment(name, action_uniforms=draws, **kw)


def fetch(e, name):
    """the last rollout's rows and ends under head-neutral keys"""
    if is_cont(name):
        d = e.rollout_gaussian_fetch()
        d["head"], d["draw"] = d["means"], d["normals"]
        ends = e.rollout_gaussian_fetch_ends()
        ends["final_head"] = ends["final_means"]
    else:
        d = e.rollout_fetch()
        d["head"], d["draw"] = d["action_dists"], d["uniforms"]
        d["env_states"] = e.rollout_fetch_states()
        ends = e.rollout_fetch_ends()
        ends["final_head"] = ends["final_dists"]
    d["ends"] = ends
    return d


def to_batch(e, name):
    e.rollout_gaussian_to_batch() if is_cont(name) else e.rollout_to_batch()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def env_blocks(d, n_envs, budget):
    """row and path ranges of each environment in a concatenated whole-episode rollout: an environment collects
    paths until its steps reach the budget"""
    lengths = d["ends"]["lengths"]
    out, p, r = [], 0, 0
    for _ in range(n_envs):
        p0, r0, cnt = p, r, 0
        while cnt < budget:
            cnt += int(lengths[p])
            p += 1
        r += cnt
        out.append((r0, r, p0, p))
    assert p == len(lengths) and r == len(d["rewards"])
    return out


# ------------------------------------------------------------------ 1. segments reproduce the whole-episode kernel
@pytest.mark.parametrize("K,T", ((5, 17), (12, 1)))
@pytest.mark.parametrize("n_envs", (1, 5))
@pytest.mark.parametrize("name", ("CartPole-v0", "Acrobot-v1", "Pendulum-v1", "MountainCarContinuous-v0"))
def test_segments_reproduce_whole_episodes(gpu_available, name, n_envs, K, T):
    e, _, env = make_engine(name)
    cont = is_cont(name)
    limit, KT = 8, K * T
    cap = KT + limit - 1
    rng = np.random.RandomState(100 * K + n_envs)
    M = KT + T + 2
    reset_u = rng.uniform(size=(n_envs, M, env.reset_draws))
    draws = rng.standard_normal((n_envs, cap, env.act_dim)) if cont else rng.uniform(size=(n_envs, cap))
    whole(e, name, n_envs=n_envs, n_timesteps=n_envs * KT, time_limit=limit, reset_uniforms=reset_u, draws=draws,
          max_episodes_per_env=M)
    w = fetch(e, name)
    blocks = env_blocks(w, n_envs, KT)
    _, _, reset, _ = S.env_fns(name)
    # the host model's segments per environment, from the device's recorded rewards, terminations and states
    models, consumed = [], []
    for i, (r0, r1, p0, p1) in enumerate(blocks):
        done = np.zeros(r1 - r0, bool)
        ends = w["ends"]
        term = ends["end_rows"][p0:p1][ends["truncated"][p0:p1] == 0]
        done[term - r0] = True
        st = w["env_states"][r0:r1]
        nxt = np.concatenate([st[1:], st[-1:]])      # the last row's successor is never read when it ended an episode
        assert r1 - r0 > KT or w["ends"]["end_rows"][p1 - 1] == r0 + KT - 1
        step, _cur = S.replay_fns(w["rewards"][r0:r1], done, nxt)
        starts = w["starts"][r0:r1]
        segs, carry, used = [], None, 0
        for j in range(K):
            # resets the environment has consumed before call j, from the whole-episode rollout's starts
            before = 0 if j == 0 else int(starts[:j * T + 1].sum())
            assert before == used
            segs.append(S.run_segment(step, reset, carry, T, limit, [None] * T, reset_u[i, before:]))
            carry = segs[-1]["carry"]
            used += segs[-1]["resets"]
            consumed.append((i, j, before))
        models.append(segs)
    f, _, _ = make_engine(name)
    got = []
    for j in range(K):
        ru = np.stack([reset_u[i, b:b + T + 1] for (i, jj, b) in consumed if jj == j])
        n, paths = segment(f, name, n_envs=n_envs, horizon=T, resume=j > 0, time_limit=limit, reset_uniforms=ru,
                           draws=np.ascontiguousarray(draws[:, j * T:(j + 1) * T]), max_episodes_per_env=T + 1)
        assert n == n_envs * T
        s = fetch(f, name)
        s["seg"] = f.rollout_segment_fetch()
        s["carry"] = f.rollout_carry()
        assert paths == len(s["seg"]["end_kind"]) == sum(len(models[i][j]["kind"]) for i in range(n_envs))
        got.append(s)
    for i, (r0, r1, _p0, _p1) in enumerate(blocks):
        for k in ROW_KEYS + ("env_states",):
            cat = np.concatenate([g[k][i * T:(i + 1) * T] for g in got])
            assert same_bits(cat, w[k][r0:r0 + KT]), (name, i, k)
    for j, g in enumerate(got):
        p = 0
        for i in range(n_envs):
            m = models[i][j]
            rows = slice(i * T, (i + 1) * T)
            assert np.array_equal(g["seg"]["step_index"][rows], m["step_index"])
            assert np.array_equal(g["starts"][rows], m["starts"])
            q = slice(p, p + len(m["kind"]))
            assert np.array_equal(g["seg"]["end_kind"][q], m["kind"])
            assert np.array_equal(g["seg"]["t0"][q], m["t0"])
            assert same_bits(g["seg"]["episode_returns"][q], np.asarray(m["episode_return"], np.float64))
            assert np.array_equal(g["ends"]["lengths"][q], m["rows"])
            assert np.array_equal(g["ends"]["end_rows"][q], i * T + m["end_row"])
            assert np.array_equal(g["ends"]["truncated"][q], m["truncated"])
            p += len(m["kind"])
            s, t, ret = m["carry"]
            assert same_bits(g["carry"]["states"][i], np.asarray(s, np.float64))
            assert g["carry"]["t"][i] == t and same_bits(g["carry"]["returns"][i], np.float64(ret))
        assert p == len(g["seg"]["end_kind"])
        assert g["carry"]["n_envs"] == n_envs and g["carry"]["env"] == env.env_id
    e.close()
    f.close()


# ------------------------------------------------------------------ 2. the Philox path
@pytest.mark.parametrize("name", ("MountainCar-v0", "Pendulum-v1"))
def test_philox_path(gpu_available, name):
    e, _, _ = make_engine(name)
    n_envs, T, seed = 5, 17, 12345
    whole(e, name, n_envs=n_envs, n_timesteps=n_envs * T, time_limit=8, seed=seed)
    w = fetch(e, name)
    blocks = env_blocks(w, n_envs, T)
    n, _ = segment(e, name, n_envs=n_envs, horizon=T, resume=False, time_limit=8, seed=seed)
    s = fetch(e, name)
    assert n == n_envs * T
    for i, (r0, _r1, _p0, _p1) in enumerate(blocks):
        for k in ROW_KEYS + ("env_states", "starts"):
            assert same_bits(s[k][i * T:(i + 1) * T], w[k][r0:r0 + T]), (name, i, k)
    e.close()


# ------------------------------------------------------------------ 3. limits across and on the boundary
def test_limit_across_calls(gpu_available):
    name = "Pendulum-v1"
    e, _, _ = make_engine(name)
    kinds, steps_at_end, t_carry = [], [], []
    for j in range(4):
        segment(e, name, n_envs=1, horizon=4, resume=j > 0, time_limit=10, seed=3 + j)
        sf, ends = e.rollout_segment_fetch(), e.rollout_gaussian_fetch_ends()
        kinds.append(list(sf["end_kind"]))
        steps_at_end.append(list(sf["t0"] + ends["lengths"]))
        t_carry.append(int(e.rollout_carry()["t"][0]))
        if j == 2:
            assert list(ends["lengths"]) == [2, 2] and list(sf["step_index"]) == [8, 9, 0, 1]
            assert list(e.rollout_gaussian_fetch()["starts"]) == [1, 0, 1, 0]
    assert kinds[:3] == [[2], [2], [1, 2]]
    assert [steps_at_end[0][0], steps_at_end[1][0], steps_at_end[2][0]] == [4, 8, 10]
    assert t_carry == [4, 8, 2, 6]
    e.close()


def test_limit_on_the_boundary(gpu_available):
    name = "Pendulum-v1"
    e, _, env = make_engine(name)
    ru = np.random.RandomState(5).uniform(size=(3, 1, 5, env.reset_draws))
    for j in range(3):
        segment(e, name, n_envs=1, horizon=4, resume=j > 0, time_limit=8, seed=3 + j, reset_uniforms=ru[j],
                max_episodes_per_env=5)
        sf = e.rollout_segment_fetch()
        c = e.rollout_carry()
        if j == 1:
            # the limit falls on the call's last step: kind 1, no kind-2 record, the carry is a reset state
            assert list(sf["end_kind"]) == [1] and list(sf["t0"]) == [4]
            assert c["t"][0] == 0 and c["returns"][0] == 0.0
            assert same_bits(c["states"][0], np.asarray(env.reset(ru[1, 0, 0]), np.float64))
        if j == 2:
            assert e.rollout_gaussian_fetch()["starts"][0] == 1 and sf["step_index"][0] == 0
            assert same_bits(e.rollout_gaussian_fetch()["env_states"][0], np.asarray(env.reset(ru[1, 0, 0])))
            assert list(sf["end_kind"]) == [2]
    e.close()


def test_termination_on_the_last_row(gpu_available):
    """CartPole-v0 carried one step before it falls over: the termination lands on a 1-step segment's only row"""
    name = "CartPole-v0"
    e, _, env = make_engine(name)
    _, step, reset, _ = S.env_fns(name)
    s, t, ret = [0.0, 0.0, 0.2, 2.0], 5, 5.0          # theta past 12 degrees after one more step, either action
    assert step(s, 0)[2] and step(s, 1)[2]
    carry_s = np.array([reset([0.5] * 4), s, reset([0.25] * 4)])
    e.set_rollout_carry(name, carry_s, [0, t, 3], [0.0, ret, 3.0])
    ru = np.random.RandomState(1).uniform(size=(3, 1, 4))
    n, paths = e.rollout_segment(name, n_envs=3, horizon=1, resume=True, seed=9, reset_uniforms=ru,
                                 max_episodes_per_env=1)
    sf, ends, c = e.rollout_segment_fetch(), e.rollout_fetch_ends(), e.rollout_carry()
    assert (n, paths) == (3, 3)
    assert list(sf["end_kind"]) == [2, 0, 2] and list(ends["truncated"]) == [1, 0, 1]
    assert list(sf["t0"]) == [0, 5, 3] and list(sf["step_index"]) == [0, 5, 3]
    assert list(sf["episode_returns"]) == [1.0, 6.0, 4.0]
    assert not ends["final_dists"][1].any() and ends["final_dists"][0].any()
    assert list(c["t"]) == [1, 0, 4] and list(c["returns"]) == [1.0, 0.0, 4.0]
    assert same_bits(c["states"][1], np.asarray(reset(ru[1, 0]), np.float64))
    e.close()


# ------------------------------------------------------------------ 4. kind-2 continuity
@pytest.mark.parametrize("name", ("Acrobot-v1", "Pendulum-v1"))
def test_kind2_continuity(gpu_available, name):
    e, th, _ = make_engine(name)
    n_envs, T = 5, 4
    segment(e, name, n_envs=n_envs, horizon=T, resume=False, time_limit=50, seed=1)
    a = fetch(e, name)
    assert list(e.rollout_segment_fetch()["end_kind"]) == [2] * n_envs
    segment(e, name, n_envs=n_envs, horizon=T, resume=True, time_limit=50, seed=2)
    b = fetch(e, name)
    for i in range(n_envs):
        assert same_bits(a["ends"]["final_obs"][i], b["obs"][i * T])
        assert same_bits(a["ends"]["final_head"][i], b["head"][i * T])
    # another theta between the calls: the observation continues, the head row is the new policy's
    th2 = th.copy()
    th2[:th2.size // 2] *= np.float32(0.5)
    e.set_flat(th2)
    segment(e, name, n_envs=n_envs, horizon=T, resume=True, time_limit=50, seed=3)
    c = fetch(e, name)
    for i in range(n_envs):
        assert same_bits(b["ends"]["final_obs"][i], c["obs"][i * T])
        assert not same_bits(b["ends"]["final_head"][i], c["head"][i * T])
    e.close()


# ------------------------------------------------------------------ 5. the VF's time feature
def test_vf_features(gpu_available):
    from trpo_amd.vf import VFNet, vf_xavier_params
    name = "Pendulum-v1"
    e, _, env = make_engine(name)
    n_envs, T = 5, 6
    F = env.obs_dim + env.act_dim + 1
    net = VFNet(F, 256)
    net.set_params(vf_xavier_params(F, (64, 64), np.random.RandomState(4)))
    segment(e, name, n_envs=n_envs, horizon=T, resume=False, time_limit=15, seed=1)
    segment(e, name, n_envs=n_envs, horizon=T, resume=True, time_limit=15, seed=2)
    segment(e, name, n_envs=n_envs, horizon=T, resume=True, time_limit=15, seed=3)   # t = 12: the limit falls inside
    d, sf = fetch(e, name), e.rollout_segment_fetch()
    assert set(sf["end_kind"]) == {1, 2} and sf["step_index"].max() == 14 and sf["step_index"][0] == 12
    to_batch(e, name)
    view = e.feed_view()
    assert view.step_index
    net.set_features_view(view)
    feat = net.feature_matrix()
    assert same_bits(feat[:, -1], (sf["step_index"] / 10.0).astype(np.float32))
    assert same_bits(feat[:, :env.obs_dim], d["obs32"]) and same_bits(feat[:, env.obs_dim:-1], d["head"])
    net.predict_tails(e.tail_view())
    tfeat = net.feature_matrix()
    ends = d["ends"]
    assert same_bits(tfeat[:, -1], ((sf["t0"] + ends["lengths"]) / 10.0).astype(np.float32))
    assert np.any(sf["t0"] > 0)
    assert same_bits(tfeat[:, :env.obs_dim], ends["final_obs"].astype(np.float32))
    # a whole-episode feed on the same engine: no step_index, the features of the path-start scan as before
    whole(e, name, n_envs=n_envs, n_timesteps=n_envs * T, time_limit=4, seed=4)
    d = fetch(e, name)
    to_batch(e, name)
    view = e.feed_view()
    assert not view.step_index
    net.set_features_view(view)
    feat = net.feature_matrix()
    net.set_features(d["obs32"], d["head"], d["starts"])
    assert same_bits(feat, net.feature_matrix())
    t = np.concatenate([np.arange(n) for n in d["ends"]["lengths"]])
    assert same_bits(feat[:, -1], (t / 10.0).astype(np.float32))
    # set_rewards on a segment feed drops its step_index with its starts
    segment(e, name, n_envs=n_envs, horizon=T, resume=True, time_limit=15, seed=5)
    d = fetch(e, name)
    to_batch(e, name)
    assert e.feed_view().step_index
    e.set_rewards(d["rewards"], d["starts"])
    assert not e.feed_view().step_index
    net.close()
    e.close()


# ------------------------------------------------------------------ 6. GAE on a segment feed
@pytest.mark.parametrize("name", ("CartPole-v0", "Pendulum-v1"))
def test_gae_on_a_segment_feed(gpu_available, name):
    from trpo_amd.vf import VFNet, vf_xavier_params
    e, _, env = make_engine(name)
    n_envs, T = 5, 6
    A = env.act_dim if is_cont(name) else env.n_actions
    net = VFNet(env.obs_dim + A + 1, 256)
    net.set_params(vf_xavier_params(env.obs_dim + A + 1, (64, 64), np.random.RandomState(4)))
    e.set_advantage_estimator("gae", LAM)
    for j in range(3):
        segment(e, name, n_envs=n_envs, horizon=T, resume=j > 0, time_limit=15, seed=1 + j)
    d, sf = fetch(e, name), e.rollout_segment_fetch()
    assert set(sf["end_kind"]) >= {1, 2}
    to_batch(e, name)
    net.predict_tails(e.tail_view())
    e.set_tail_values_in_place()
    tails = e.tail_values()
    ends = d["ends"]
    cut = ends["truncated"] == 1
    assert np.all(tails[ends["end_rows"][cut]] != 0.0) and np.count_nonzero(tails) == int(cut.sum())
    base = np.random.RandomState(2).uniform(-5, 5, n_envs * T)
    e.set_baseline(base)
    ret, adv = e.compute_advantages(GAMMA)
    A_ref, R_ref, _ = gae_ref(d["rewards"], base, GAMMA, LAM, d["starts"], tails)
    print(f"{name}: returns max rel error {np.max(np.abs(ret - R_ref) / np.abs(R_ref)):.3e}")
    np.testing.assert_allclose(ret, R_ref, rtol=1e-13)
    np.testing.assert_allclose(adv, O.standardize(A_ref), rtol=1e-11, atol=1e-12)
    net.close()
    e.close()


# ------------------------------------------------------------------ 7. the carry survives other calls
@pytest.mark.parametrize("name", ("MountainCar-v0", "MountainCarContinuous-v0"))
def test_carry_survives_other_calls(gpu_available, name):
    e, th, _ = make_engine(name)
    f, _, _ = make_engine(name)
    n_envs, T = 5, 7
    for g in (e, f):
        segment(g, name, n_envs=n_envs, horizon=T, resume=False, time_limit=20, seed=1)
    c0 = e.rollout_carry()
    # an evaluation rollout that needs larger buffers, and a set_flat, between the two segments
    whole(e, name, n_envs=7, n_timesteps=7 * 40, time_limit=30, seed=8, train=False)
    e.set_flat(th * np.float32(0.5))
    e.set_flat(th)
    c1 = e.rollout_carry()
    for k in ("states", "t", "returns"):
        assert same_bits(c0[k], c1[k]), k
    assert (c1["env"], c1["n_envs"]) == (c0["env"], n_envs)
    for g in (e, f):
        segment(g, name, n_envs=n_envs, horizon=T, resume=True, time_limit=20, seed=2)
    a, b = fetch(e, name), fetch(f, name)
    for k in ROW_KEYS + ("env_states", "starts"):
        assert same_bits(a[k], b[k]), k
    assert same_bits(e.rollout_segment_fetch()["step_index"], np.tile(np.arange(T, 2 * T), n_envs))
    e.clear_rollout_carry()
    from trpo_amd._lib import EngineError
    with pytest.raises(EngineError, match="rc=-4"):
        e.rollout_carry()
    e.close()
    f.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals(gpu_available):
    from trpo_amd import Engine, xavier_theta
    from trpo_amd._lib import EngineError
    name = "CartPole-v0"
    e, _, env = make_engine(name)

    def unchanged(before_rows, before_carry):
        after = e.rollout_fetch()
        for k in before_rows:
            assert same_bits(before_rows[k], after[k]), k
        if before_carry is None:
            with pytest.raises(EngineError, match="rc=-4"):
                e.rollout_carry()
        else:
            c = e.rollout_carry()
            for k in ("states", "t", "returns"):
                assert same_bits(before_carry[k], c[k]), k

    # resume without a carry; segment_fetch after a whole-episode rollout
    e.rollout(name, n_envs=2, n_timesteps=20, time_limit=8, seed=1)
    rows = e.rollout_fetch()
    with pytest.raises(EngineError, match="rc=-4.*carry"):
        e.rollout_segment(name, n_envs=2, horizon=4, resume=True)
    unchanged(rows, None)
    with pytest.raises(EngineError, match="rc=-4.*not a segment"):
        e.rollout_segment_fetch()
    unchanged(rows, None)
    # a carry of other n_envs / another environment
    e.rollout_segment(name, n_envs=2, horizon=4, resume=False, time_limit=8, seed=2)
    rows, carry = e.rollout_fetch(), e.rollout_carry()
    with pytest.raises(EngineError, match="rc=-4.*n_envs 2"):
        e.rollout_segment(name, n_envs=3, horizon=4, resume=True, time_limit=8)
    unchanged(rows, carry)
    # a carried t at or past ep_max (a shorter limit than the carry was collected under)
    with pytest.raises(EngineError, match="rc=-1.*carries t = 4"):
        e.rollout_segment(name, n_envs=2, horizon=4, resume=True, time_limit=4)
    with pytest.raises(EngineError, match="rc=-1.*carries t = 4"):
        e.rollout_segment(name, n_envs=2, horizon=4, resume=True, time_limit=8, max_pathlength=3)
    unchanged(rows, carry)
    # injected resets without room for every reset of the call
    ru = np.full((2, 4, 4), 0.5)
    with pytest.raises(EngineError, match="rc=-1.*max_episodes_per_env"):
        e.rollout_segment(name, n_envs=2, horizon=4, resume=False, reset_uniforms=ru, max_episodes_per_env=4)
    ru3 = np.full((2, 3, 4), 0.5)
    with pytest.raises(EngineError, match="rc=-1.*max_episodes_per_env"):
        e.rollout_segment(name, n_envs=2, horizon=4, resume=True, time_limit=8, reset_uniforms=ru3,
                          max_episodes_per_env=3)
    unchanged(rows, carry)
    # the wrong head for the call; an environment of other dims
    with pytest.raises(EngineError, match="rc=-4.*gaussian engine"):
        e.rollout_gaussian_segment("Pendulum-v1", n_envs=2, horizon=4)
    with pytest.raises(EngineError, match="rc=-1.*Acrobot-v1 needs obs_dim 6"):
        e.rollout_segment("Acrobot-v1", n_envs=2, horizon=4)
    with pytest.raises(EngineError, match="rc=-1"):
        e.set_rollout_carry("MountainCar-v0", np.zeros((2, 2)), [0, 0], [0.0, 0.0])
    unchanged(rows, carry)
    # a carry of another environment that has the engine's dims cannot exist for CartPole's (4, 2); the Gaussian
    # pair shares state_dim 2 but not obs_dim, so the environment check of resume is reached through set_rollout_carry
    g = Engine(2, HIDDEN, 1, max_rows=64, dist="gaussian")
    g.set_flat(np.concatenate([xavier_theta(2, HIDDEN, 1, np.random.RandomState(1)), np.zeros(1, np.float32)]))
    with pytest.raises(EngineError, match="rc=-4.*categorical engine"):
        g.rollout_segment(name, n_envs=2, horizon=4)
    g.rollout_gaussian_segment("MountainCarContinuous-v0", n_envs=2, horizon=4, time_limit=8)
    with pytest.raises(EngineError, match="rc=-1.*Pendulum-v1 needs obs_dim 3"):
        g.rollout_gaussian_segment("Pendulum-v1", n_envs=2, horizon=4, resume=True)
    assert g.rollout_carry()["t"].tolist() == [4, 4]
    # more rows than max_rows: refused by to_batch, as for any rollout
    g.rollout_gaussian_segment("MountainCarContinuous-v0", n_envs=5, horizon=13, time_limit=8)
    with pytest.raises(EngineError, match="max_rows"):
        g.rollout_gaussian_to_batch()
    assert len(g.rollout_segment_fetch()["step_index"]) == 65
    g.close()
    e.close()
