"""The fp64 oracle of tests/ddqn_fixtures.py, settled without a GPU: (A) against torch autograd in fp64,
(B) against the CPU learner's head (``TorchBackend(torch.float32).head``), and (C) the conditions on the
fixtures under which every row of every problem can be compared with an fp32 kernel."""
import numpy as np
import pytest
import torch

import ddqn_fixtures as F

PROBLEMS = F.head_problems()
IDS = ["-".join(str(x) for x in p) for p in PROBLEMS]


# ------------------------------------------------------------ A. oracle vs autograd
@pytest.mark.parametrize("B,A,HS,split,case", PROBLEMS, ids=IDS)
def test_oracle_matches_fp64_autograd(B, A, HS, split, case):
    """The scalar sum_b w_b l_b grad_scale with the target G detached, differentiated by autograd: its
    gradient at the activations times (h > 0) is dH, at the value output dhead[:, 0], at the advantage outputs
    dhead[:, 1:], at the online head's parameters g."""
    fx = F.fixture(B, A, HS, split)
    c = F.case_inputs(fx, case)
    r = F.oracle(B, A, HS, split, case)
    Hon, Htg = F.join64(fx["Hon"], fx["Hon_lo"]), F.join64(fx["Htg"], fx["Htg_lo"])
    P = {k: v.double().clone().requires_grad_(True) for k, v in c["Pon"].items()}
    T = {k: v.double() for k, v in c["Ptg"].items()}
    h = Hon[:B].clone().requires_grad_(True)
    ar, act = torch.arange(B), c["act"].long()

    def streams(x, Q):
        return x[:, :HS] @ Q["wv"] + Q["bv"], x[:, HS:] @ Q["wa"].t() + Q["ba"]

    with torch.no_grad():
        vn, an = streams(Hon[B:], P)
        vg, ag = streams(Htg, T)
        qn, qg = vn[:, None] + an - an.mean(1, keepdim=True), vg[:, None] + ag - ag.mean(1, keepdim=True)
        astar = torch.tensor([min(j for j in range(A) if qn[b, j] == qn[b].max()) for b in range(B)])
        G = c["rew"].double() + c["gam"].double() * qg[ar, astar]
    v, a = streams(h, P)
    v.retain_grad()
    a.retain_grad()
    delta = G - (v[:, None] + a - a.mean(1, keepdim=True))[ar, act]
    k = c["kappa"]
    lval = 0.5 * delta ** 2 if not c["huber"] else torch.where(delta.abs() <= k, 0.5 * delta ** 2, k * (delta.abs() - 0.5 * k))
    w = torch.ones(B, dtype=torch.float64) if c["isw"] is None else c["isw"].double()
    (w * lval / B).sum().backward()
    tol = dict(rtol=0, atol=1e-12)
    assert torch.equal(astar, r["astar"])
    torch.testing.assert_close(delta.detach(), r["delta"], **tol)
    torch.testing.assert_close((w * lval).detach(), r["loss"], **tol)
    torch.testing.assert_close(h.grad, r["dH_pre"], **tol)
    torch.testing.assert_close(h.grad * (Hon[:B] > 0), r["dH"], **tol)
    torch.testing.assert_close(v.grad, r["dhead"][:, 0], **tol)
    torch.testing.assert_close(a.grad, r["dhead"][:, 1:], **tol)
    for name in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(P[name].grad, r["g"][name], **tol)
    torch.testing.assert_close(r["td"], r["delta"].abs(), **tol)
    torch.testing.assert_close(r["dq"], r["dhead"][:, 0], **tol)


# -------------------------------------------------- B. oracle vs the CPU learner's head
@pytest.mark.parametrize("B,A,HS,split,case", PROBLEMS, ids=IDS)
def test_oracle_matches_torch_backend_head(B, A, HS, split, case):
    """``TorchBackend(torch.float32).head`` and ``head_wgrad`` on the same planes, at the tolerances of
    tests/test_gpu_kernels.py test_ddqn_head_kernel_vs_torch: the CPU learner's head and the oracle are the
    same function."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float32)
    fx = F.fixture(B, A, HS, split)
    c = F.case_inputs(fx, case)
    r = F.oracle(B, A, HS, split, case)
    td, loss, q = torch.zeros(B), torch.zeros(B), torch.zeros(B, A)
    dH, dH_lo, dhead = torch.zeros(B, 2 * HS), torch.zeros(B, 2 * HS), torch.zeros(B, A + 1)
    be.head(fx["Hon"], fx["Htg"], c["Pon"], c["Ptg"], c["act"], c["rew"], c["gam"], c["isw"], c["huber"], c["kappa"],
            1.0 / B, td, loss, dH, dhead, q_out=q, lo=(fx["Hon_lo"], fx["Htg_lo"], dH_lo) if split else None)
    g = {k: torch.zeros_like(v) for k, v in c["Pon"].items()}
    be.head_wgrad(fx["Hon"], dhead, g, Hon_lo=fx["Hon_lo"])
    f = lambda t: t.float()                                              # noqa: E731
    torch.testing.assert_close(td, f(r["td"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(loss, f(r["loss"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dH + dH_lo, f(r["dH"]), rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(dhead, f(r["dhead"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(q, f(r["q"]), rtol=1e-4, atol=1e-4)
    for k in g:
        torch.testing.assert_close(g[k], f(r["g"][k]), rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------- C. fixture conditions
@pytest.mark.parametrize("B,A,HS,split,case", PROBLEMS, ids=IDS)
def test_head_fixture_conditions(B, A, HS, split, case):
    """Every row's top-2 gap of q_n and every row's ||delta| - kappa| exceed 2e-3 (20 x the 1e-4 q / td
    tolerance: an fp32 kernel cannot take the other branch, so no row is excluded from any comparison); plain
    problems of B >= 5 hold a row per Huber branch, of B >= 8 a terminal row."""
    r = F.oracle(B, A, HS, split, case)
    assert F.conditions(r, B, F.fixture(B, A, HS, split)["gam"], case) == []
    fx = F.fixture(B, A, HS, split)
    if case == "terminal":
        qsa = r["q"][torch.arange(B), fx["act"].long()]
        torch.testing.assert_close(r["td"], (fx["rew"].double() - qsa).abs(), rtol=0, atol=1e-12)
    if case == "tie_all":
        assert bool((r["q_n"] == r["q_n"][:, :1]).all()) and bool((r["astar"] == 0).all())
        assert bool((r["q"] == r["q"][:, :1]).all())
    if case == "tie_pair":
        assert bool((r["astar"] == 1).all()) and bool((r["q_n"][:, 1] == r["q_n"][:, 2]).all())
        # the second of the tied maxima would give another target: a kernel that took it is told apart
        live = fx["gam"] > 0
        assert int(((r["q_g"][live, 1] - r["q_g"][live, 2]).abs() > 100 * 1e-4).sum()) >= 10
    if case == "zero_isw":
        z = torch.arange(B) % 3 == 0
        assert bool((r["loss"][z] == 0).all()) and bool((r["dhead"][z] == 0).all()) and bool((r["dH"][z] == 0).all())
        assert bool((r["dhead"][~z, 0] != 0).all())


def test_seed_2_misses_the_bar_at_some_problems():
    """Why the seeds are per-width constants: with generator seed 2 the (33, 4) problem at HS = 256 has a
    top-2 gap below the bar."""
    r = F.oracle(33, 4, 256, False, "plain", seed=2)
    assert r["gap"] < F.MARGIN


@pytest.mark.parametrize("B,HS,K,split", F.FC_PROBLEMS)
def test_fc_fixture_conditions(B, HS, K, split):
    """The same two margins on the head oracle fed with the fp64 fc output, and with that output rounded as
    the fc kernel stores it (what the GPU test's oracle is fed with, up to fp32 summation error)."""
    for h in (F.fc_h64(B, HS, K, split), F.fc_h_rounded(B, HS, K, split)):
        r = F.fc_head_oracle(B, HS, K, split, h)
        assert r["gap"] > F.MARGIN and r["kmargin"] > F.MARGIN, (r["gap"], r["kmargin"])
    assert bool((F.fc_h64(B, HS, K, split) > 0).any(1).all())


@pytest.mark.parametrize("HS", F.HIDDEN)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("E,A", F.ACTOR_EA)
def test_actor_fixture_conditions(E, A, HS, split):
    assert F.actor_oracle(E, A, HS, split)["gap"] > F.MARGIN


SEEDS = (5, (1 << 32) + 12345)
CTRS = (0, 7, (1 << 40) + 3)


def test_rng_mirror_properties():
    """What the exact comparison with the mirror is worth, stated on the mirror: at E = 257, A = 18 both
    branches occur and the explored rows take >= 10 distinct actions; the forced rows (eps = the row's own
    u) are greedy; rows of one launch use different draws; ctr and ctr + 1 give different action vectors at
    eps = 1; draws lie in [0, 1)."""
    from apex_dqn_amd.replay.gpu_replay import apex_uniform
    E, A = 257, 18
    raw = F.actor_fixture(E, A)["eps"]
    for seed in SEEDS:
        for ctr in CTRS:
            eps, u, r, explore, a_rand = F.actor_draws(E, A, seed, ctr, raw)
            assert explore.any() and (~explore).any()
            assert len(set(a_rand[explore].tolist())) >= 10
            assert not explore[0] and explore[1] and not explore[F.actor_forced_rows(E)].any()
            assert (u >= 0).all() and (u < 1).all() and (r >= 0).all() and (r < 1).all()
            assert len(set(u.tolist())) > E // 2 and len(set(r.tolist())) > E // 2 and not np.array_equal(u, r)
            assert a_rand.min() >= 0 and a_rand.max() <= A - 1
            nxt = F.actor_draws(E, A, seed, ctr + 1, raw)
            assert not np.array_equal(a_rand, nxt[4]) and not np.array_equal(u, nxt[1])
        assert not np.array_equal(F.actor_draws(E, A, seed, 7, raw)[1], F.actor_draws(E, A, seed + 1, 7, raw)[1])
    # the counter's high bits and the seed's reach the draw
    i = np.arange(8, dtype=np.uint64)
    assert not np.array_equal(apex_uniform(5, 3, i), apex_uniform(5, (1 << 40) + 3, i))
    assert not np.array_equal(apex_uniform(12345, 3, i), apex_uniform((1 << 32) + 12345, 3, i))
