"""The update's decision branches on every engine path: where CG stops (the device flags fl->done[it] that every
later FVP launch receives as `skip`), which step fraction 2^-k the line search accepts (trial 0 inside the captured
graph, the others outside it) or none, and whether the step is undone (kl_after > 2 max_kl).

The cases are the table of tests/update_outcomes_ref.py: engineered with max_kl, a residual_tol between two rdotr of
the float64 trace, an advantage scale and a perturbed old policy, each admitted only where the float64 reference
clears every decision with margin and float32 decides the same (tests/test_update_outcomes_ref.py proves that on
the CPU), so the engine must take the same branches and land within 1e-5 of the float64 values.  The paths
(update_outcomes_ref.PATHS): fused16, fused = 2, fused = 0 and chain = 0 at C3 dims, the per-layer path at C4 dims
with a partial last row tile, C5 dims, three hidden layers, the Gaussian head at two sizes, the fvp_subsample child
(which borrows its owner's scalar block and done flags) and a one-rank RCCL communicator.

Bars, in every case: vectors assert_vec_close at 1e-5; shs, lm, rate 1e-5 relative; the losses after the step the
bars of test_update_vs_golden.  Only for the losses at the accepted point of a large-max_kl case (max_kl >= 10 and
k >= 0), where the softmax is saturated and float32 cannot always meet 1e-5, the bar is test_gpu_fused16_hard.py's
max(1e-5, 4 x the float32 reference's own error against float64); margin lines mark those with `*` and go to
$TRPO_MARGIN_LOG through log_margin.

test_one_graph_changing_outcomes replays one captured update graph (one residual_tol, one row count) across updates
whose stop iteration, k, acceptance and revert all change from one replay to the next, and requires each to be
bitwise the same case on a fresh engine without graphs: cg_init_finish must re-zero the done flags, shs_finish must
reset accepted / k / reverted, ls_finalize must pick its branch from this replay's scalars.  The engine has no
replay counter: like the other graph tests, this one cannot tell a replay from the quiet eager fallback that
run_prefix takes when hipGraphInstantiate fails; it holds whichever ran to the eager values.
"""
import contextlib

import numpy as np
import pytest

import update_outcomes_ref as U
from conftest import assert_vec_close, rel_l2
from test_gpu_fused16_hard import log_margin

pytestmark = pytest.mark.gpu
REL = 1e-5
LARGE_MAX_KL = 10.0     # the default is 0.01; every engineered k > 0 case of the table is above 27


@contextlib.contextmanager
def options(pairs):
    from trpo_amd._lib import get_option, set_option
    saved = {name: get_option(name) for name, _ in pairs}
    try:
        for name, value in pairs:
            set_option(name, value)
        yield
    finally:
        for name, value in saved.items():
            set_option(name, value)


def make_engine(path):
    from trpo_amd import Engine
    p = U.PATHS[path]
    obs, hidden, A = p.dims
    e = Engine(obs, hidden, A, max_rows=p.n, dist="gaussian" if p.head == "gauss" else "categorical")
    if p.comm:
        e.comm_init(Engine.comm_unique_id(), 0, 1)
        assert e.comm_info()["transport"] == "rccl"
    if p.stride > 1:
        e.set_fvp_subsample(p.stride)
    return e


def feed_engine(e, fd, adv_scale):
    adv = U.scaled_advant(fd, adv_scale)
    e.set_flat(fd.theta)
    if fd.head == "gauss":
        e.set_batch_gaussian(fd.X, fd.actions, adv, fd.old, fd.old_logstd)
    else:
        e.set_batch(fd.X, fd.actions, adv, fd.old)


def run_update(e, case, tol):
    """feed the case, run one update -> (stats, {vector name: array})"""
    from trpo_amd import UpdateParams
    from trpo_amd._lib import VEC_FULLSTEP, VEC_G, VEC_STEPDIR, VEC_THETA_LS
    fd = U.path_feed(case.path, case.seed, case.perturbed)
    feed_engine(e, fd, case.adv_scale)
    st = e.update(UpdateParams(cg_iters=U.CG_ITERS, residual_tol=tol, cg_damping=U.PATHS[case.path].damping,
                               max_kl=case.max_kl))
    vecs = {"g": e.get_vector(VEC_G), "stepdir": e.get_vector(VEC_STEPDIR), "fullstep": e.get_vector(VEC_FULLSTEP),
            "theta_ls": e.get_vector(VEC_THETA_LS), "theta_new": e.get_flat()}
    return st, vecs


def run_case(case, graphs=None):
    """the case on a fresh engine of its path"""
    t = U.reference(case.id)
    opts = U.PATHS[case.path].options + ((("graphs", graphs),) if graphs is not None else ())
    with options(opts):
        e = make_engine(case.path)
        try:
            return run_update(e, case, t.tol)
        finally:
            e.close()


def check_against_reference(case, st, vecs):
    """the assertions of one case against the float64 Trace; returns the margin line"""
    t, t32 = U.reference(case.id), U.reference(case.id, False)
    fd = U.path_feed(case.path, case.seed, case.perturbed)
    what = case.id
    assert (st["cg_iters"], st["k"], bool(st["reverted"])) == t.outcome == case.expect, (what, st)
    worst = []

    # the float32 rule holds for the losses at an accepted point of a large-max_kl case alone (saturated softmax,
    # or a Gaussian ratio far out on its exponential); everything else is held to the flat bars
    saturated = case.max_kl >= LARGE_MAX_KL and t.k >= 0

    def vec(name):
        got, want = vecs[name], getattr(t, name)
        assert_vec_close(got, want, REL, f"{what} {name}")
        worst.append(f"{name} {rel_l2(got, want):.1e}")

    def scalar(name, got, want, want32=None, abs_=0.0):
        # |got - want| <= max(1e-5 |want|, abs_) and, with want32, 4 x the float32 reference's own error; at k = -1
        # surr and kl are the losses at theta_0, zero but for rounding: test_update_vs_golden's absolute bar carries them
        want = float(want)
        err32 = abs(float(want32) - want) if want32 is not None else 0.0
        tol = max(REL * abs(want), abs_, 4.0 * err32)
        assert abs(got - want) <= tol, (what, name, got, want, tol)
        worst.append(f"{name} {abs(got - want):.1e}/{tol:.0e}" + ("*" if err32 and tol == 4.0 * err32 else ""))

    for name in ("stepdir", "fullstep", "theta_ls", "theta_new"):
        vec(name)
    for name in ("shs", "lm", "rate"):
        scalar(name, st[name], getattr(t, name))
    la, la32 = t.losses_after, (t32.losses_after if saturated else (None, None, None))
    scalar("surr_after", st["surr_after"], la[0], la32[0], 1e-7)
    scalar("kl_after", st["kl_after"], la[1], la32[1], 1e-7)
    scalar("ent_after", st["ent_after"], la[2], la32[2])
    assert np.all(np.isfinite([st[k] for k in ("shs", "lm", "rate", "surr_after", "kl_after", "ent_after", "rdotr")]))
    for name, v in vecs.items():
        assert np.all(np.isfinite(v)), (what, name)
    if t.k == -1 or t.reverted:
        assert vecs["theta_new"].tobytes() == fd.theta.tobytes(), f"{what}: theta is not bitwise theta_0"
    if t.k == -1:
        assert vecs["theta_ls"].tobytes() == fd.theta.tobytes()
        for name in ("surr", "kl", "ent"):
            assert np.float32(st[name + "_after"]).tobytes() == np.float32(st[name + "_before"]).tobytes(), (what, name)
    if t.reverted:
        assert vecs["theta_ls"].tobytes() != fd.theta.tobytes()     # the accepted point is kept there
    return f"update outcome {what}: {t.outcome} tol {t.tol:.3e} max_kl {case.max_kl:g}: " + ", ".join(worst)


@pytest.mark.parametrize("case_id", U.IDS)
def test_outcome_vs_reference(gpu_available, case_id):
    case = U.BY_ID[case_id]
    st, vecs = run_case(case)
    log_margin(check_against_reference(case, st, vecs))


@pytest.mark.parametrize("path", [p for p in U.PATHS if not p.startswith("mrank")])
def test_path_is_the_one_named(gpu_available, path):
    """The profile tags of one eager update show the kernels the path is here for.  The engine has no tag for the
    rh1_planes option: on the C4 path it is implied by fvp_rfwd01 + fvp_rbwdwg_l1 (its writer and its reader) with
    the option at its default, not confirmed by a tag of its own."""
    from trpo_amd import UpdateParams
    p = U.PATHS[path]
    fd = U.path_feed(path, 7)
    with options(p.options + (("graphs", 0),)):
        e = make_engine(path)
        try:
            e.profile_enable()
            feed_engine(e, fd, 1.0)
            e.update(UpdateParams(cg_iters=U.CG_ITERS, residual_tol=0.0, cg_damping=p.damping))
            seen = set(e.profile_query())
        finally:
            e.close()
    log_margin(f"update outcome path {path}: tags {sorted(seen)}")
    assert p.tags, path
    assert set(p.tags) <= seen, f"{path}: paths not taken: {sorted(set(p.tags) - seen)} (seen {sorted(seen)})"
    assert not set(p.no_tags) & seen, f"{path}: took {sorted(set(p.no_tags) & seen)}"


KEYS = ("cg_iters", "k", "reverted", "shs", "lm", "rate", "surr_before", "kl_before", "ent_before", "surr_after",
        "kl_after", "ent_after", "rdotr", "gdotstepdir")


@pytest.mark.parametrize("path", list(U.GRAPH_STEPS))
def test_one_graph_changing_outcomes(gpu_available, path):
    tol, _ = U.GRAPH_STEPS[path]
    steps = [c for c in U.GRAPH_CASES if c.path == path]
    # each step on a fresh engine without graphs: the values every replay must reproduce bit for bit
    fresh = {}
    for c in steps:
        assert U.reference(c.id).tol == tol
        st, vecs = run_case(c, graphs=0)
        log_margin(check_against_reference(c, st, vecs))
        fresh[c.id] = (st, vecs)
    assert len({tuple(fresh[c.id][0][k] for k in ("cg_iters", "k", "reverted")) for c in steps}) == len(steps)
    with options(U.PATHS[path].options + (("graphs", 1),)):
        e = make_engine(path)
        try:
            seq = steps * 2          # the 1st update runs eagerly, the 2nd captures, the other ten replay
            assert len(seq) >= 8
            for i, c in enumerate(seq):
                st, vecs = run_update(e, c, tol)
                st0, vecs0 = fresh[c.id]
                for k in KEYS:
                    assert np.float64(st[k]).tobytes() == np.float64(st0[k]).tobytes(), (path, i, c.id, k, st[k], st0[k])
                for name in ("theta_new", "stepdir", "theta_ls", "fullstep", "g"):
                    assert vecs[name].tobytes() == vecs0[name].tobytes(), f"{path} update {i} ({c.id}): {name}"
        finally:
            e.close()


CG_PATHS = ("p4_layers", "p7_gauss_small", "p7_gauss_c4", "p8_sub3_fused16", "p8_sub3_layers")


@pytest.mark.parametrize("path", CG_PATHS)
def test_engine_cg_stops_where_the_trace_does(gpu_available, path):
    """Engine.cg(b, 10, tol, damping) at three tols of the float64 trace: the same iteration count, x within 1e-5"""
    p = U.PATHS[path]
    fd = U.path_feed(path, 7)
    cg = U.cg_trace(path, 7, False, 1.0)
    stops = U.admissible_stops(cg.rdotr)
    assert len(stops) >= 3, (path, stops)
    b = (-cg.g).astype(np.float32)
    with options(p.options):
        e = make_engine(path)
        try:
            feed_engine(e, fd, 1.0)
            for j in (stops[0], stops[len(stops) // 2], stops[-1]):
                tol = U.tol_for_stop(cg.rdotr, j)
                x, it = e.cg(b, U.CG_ITERS, tol, p.damping)
                assert it == j, (path, j, it, tol)
                assert_vec_close(x, cg.xs[j - 1], REL, f"{path} cg stop {j}")
            x, it = e.cg(b, U.CG_ITERS, 0.0, p.damping)
            assert it == U.CG_ITERS
            assert_vec_close(x, cg.xs[-1], REL, f"{path} cg full")
        finally:
            e.close()


@pytest.mark.parametrize("case", U.AGENT_CASES, ids=[c.id for c in U.AGENT_CASES])
def test_agent_update_and_stepwise(gpu_available, case):
    """TRPOAgent.update and update_stepwise (max_kl through config) agree with each other and with the reference"""
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    t, t32 = U.reference(case.id), U.reference(case.id, False)
    fd = U.path_feed(case.path, case.seed, case.perturbed)
    obs, hidden, A = U.PATHS[case.path].dims
    batch = {"state": fd.X, "action": fd.actions, "action_dist": fd.old, "advant": U.scaled_advant(fd, 1.0)}
    cfg = dict(CONFIG, max_kl=case.max_kl)
    a1 = TRPOAgent(obs, A, hidden, max_rows=fd.X.shape[0], theta=fd.theta, config=cfg)
    a2 = TRPOAgent(obs, A, hidden, max_rows=fd.X.shape[0], theta=fd.theta, config=cfg)
    s1 = a1.update(batch)
    s2 = a2.update_stepwise(batch)
    assert (s1["cg_iters"], s1["k"], bool(s1["reverted"])) == t.outcome
    assert s2["reverted"] == t.reverted
    for name, a in (("update", a1), ("update_stepwise", a2)):
        if t.reverted:
            assert a.gf().tobytes() == fd.theta.tobytes(), name
        else:
            assert_vec_close(a.gf(), t.theta_new, REL, f"{case.id} {name} theta_new")
    assert_vec_close(a1.gf(), a2.gf(), REL, "fused vs stepwise")
    for name, want in (("shs", t.shs), ("lm", t.lm)):
        assert s1[name] == pytest.approx(want, rel=REL) and s2[name] == pytest.approx(want, rel=REL), name
    # kl_after at the accepted point: the float32 rule where max_kl is large (check_against_reference)
    rel = REL
    if case.max_kl >= LARGE_MAX_KL and t.k >= 0:
        rel = max(REL, 4.0 * abs(t32.kl_after - t.kl_after) / abs(t.kl_after))
    for s_ in (s1, s2):
        assert s_["kl_after"] == pytest.approx(t.kl_after, rel=rel, abs=1e-7)


# ---- two ranks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c.id for c in U.MRANK_CASES])
def test_two_ranks_take_the_same_branches(gpu_available, case_id):
    """tools/mrank_check.py with the case's max_kl / residual_tol on its own feed (synthetic_batch seed 3): ranks
    bitwise identical, graph replays equal to eager, and cg_iters / k / reverted those of one rank, which the
    tool is told to expect from the CPU table."""
    from test_gpu_parity import run_mrank
    c = U.BY_ID[case_id]
    t = U.reference(case_id)
    dims = {tuple(map(str, (v[0], v[1], v[2]))): k for k, v in (("c3", U.C3), ("c4", U.C4))}[
        tuple(map(str, U.PATHS[c.path].dims))]
    run_mrank("--host-allreduce", "--graphs", "--dims", dims, "--rows", str(U.PATHS[c.path].n),
              "--max-kl", repr(c.max_kl), "--residual-tol", repr(t.tol), "--adv-scale", repr(c.adv_scale),
              "--expect", ",".join(str(int(x)) for x in t.outcome), timeout=300)
