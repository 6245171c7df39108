"""Implicit quantile (IQN) head without a GPU: the tau mirror (learner/iqn.py), ``iqn_loss``
(learner/losses.py), the torch backend's head and weight gradient (ops/fused_ops.py) against
autograd, and the fixtures and tolerances tests/test_gpu_iqn.py relies on."""
import math

import numpy as np
import pytest
import torch

import iqn_fixtures as F
from apex_dqn_amd.learner import iqn
from apex_dqn_amd.learner.losses import iqn_loss, quantile_huber_loss, quantile_huber_terms
from apex_dqn_amd.replay.gpu_replay import apex_uniform


# ------------------------------------------------------------------ the mirror
def test_mirror_is_deterministic_in_range_and_keyed():
    s = iqn.iqn_seed(7)
    a, b = iqn.learner_taus(s, 3, 16, 8), iqn.learner_taus(s, 3, 16, 8)
    assert a.dtype == torch.float32 and a.shape == (16, 3, 8) and torch.equal(a, b)
    big = iqn.learner_taus(s, 0, 512, 64)
    assert float(big.min()) >= 0.0 and float(big.max()) < 1.0
    assert abs(float(big.mean()) - 0.5) < 0.01
    # the three sets of a row, two updates, two seeds: all different draws
    assert not torch.equal(a[:, 0], a[:, 1]) and not torch.equal(a[:, 1], a[:, 2]) and not torch.equal(a[:, 0], a[:, 2])
    assert not torch.equal(a, iqn.learner_taus(s, 4, 16, 8))
    assert not torch.equal(a, iqn.learner_taus(iqn.iqn_seed(8), 3, 16, 8))
    # N does not move a draw: the first fractions of a longer set are the shorter set
    assert torch.equal(iqn.learner_taus(s, 3, 16, 64)[:, :, :8], a)
    # actors: groups and calls differ, and differ from the learner's stream of the same index
    g0, g1 = iqn.actor_taus(s, 5, 0, 12, 32), iqn.actor_taus(s, 5, 1, 12, 32)
    assert g0.shape == (12, 32) and not torch.equal(g0, g1) and not torch.equal(g0, iqn.actor_taus(s, 6, 0, 12, 32))
    assert torch.equal(g0, iqn.actor_taus(s, 5, 0, 12, 32))
    assert not torch.equal(g0[:, :8], iqn.learner_taus(s, 5, 12, 8)[:, 0])


def test_seed_q_is_its_own_word():
    from apex_dqn_amd.learner.noisy import noise_seed
    assert iqn.iqn_seed(1) != noise_seed(1) and iqn.iqn_seed(1) != 1 and iqn.iqn_seed(1) != iqn.iqn_seed(2)
    assert 0 <= iqn.iqn_seed(2 ** 63 + 5) < 2 ** 63


def test_mirror_equals_apex_uniform_by_hand():
    s = iqn.iqn_seed(11)
    t = iqn.learner_taus(s, 9, 8, 5)
    for (b, st, k) in ((0, 0, 0), (3, 2, 4), (7, 1, 2)):
        assert float(t[b, st, k]) == float(apex_uniform(s, 64 * 9, (3 * b + st) * 64 + k))
    a = iqn.actor_taus(s, 4, 3, 6, 7)
    for (e, k) in ((0, 0), (5, 6), (2, 3)):
        assert float(a[e, k]) == float(apex_uniform(s, 64 * 4 + 2 + 3, e * 64 + k))
    assert torch.equal(iqn.midpoint_taus(4), torch.tensor([0.125, 0.375, 0.625, 0.875]))


def test_kernel_cosine_formula_meets_the_fp64_definition():
    """cos(pi i tau) is defined in fp64 at the fp32 tau; the fp32 product i tau rounds.  The kernel's form
    (csrc/iqn_head.hip ``iqn_cos``): p = fl(i tau), r = the exact residual (one fma), cos(pi p) - pi r
    sin(pi p).  Emulated here with fp64 sin / cos of the fp32 p: the first-order term leaves <= 1e-7;
    without it the error reaches 1e-5."""
    tau = iqn.learner_taus(iqn.iqn_seed(3), 0, 64, 64).reshape(-1).numpy()
    i = np.arange(64, dtype=np.float32)[None, :]
    p = (i * tau[:, None]).astype(np.float32)
    r = i.astype(np.float64) * tau[:, None].astype(np.float64) - p.astype(np.float64)       # exact in fp64
    ref = iqn.cos_features(torch.from_numpy(tau)).numpy()
    plain = np.cos(np.pi * p.astype(np.float64))
    fixed = plain - np.pi * r * np.sin(np.pi * p.astype(np.float64))
    assert np.abs(fixed - ref).max() <= 1e-7
    assert np.abs(plain - ref).max() > 1e-6


# -------------------------------------------------------------------- the loss
def test_iqn_loss_by_hand():
    """B = 2, N = 2, kappa = 1: row 0 has one |u| <= kappa entry, one |u| > kappa entry and two u < 0
    entries; row 1 is terminal (Gamma = 0: T_j = R)."""
    kappa = 1.0
    theta_t = torch.tensor([[[0.0, 1.0], [9.0, 9.0]], [[5.0, 5.0], [2.0, 4.0]]], dtype=torch.float64)   # [B, A, N]
    tau_t = torch.tensor([[0.25, 0.5], [0.1, 0.9]], dtype=torch.float64)
    q_next = torch.tensor([[0.0, 1.0], [3.0, 3.0]], dtype=torch.float64)        # a* = 1, then the first maximum 0
    theta_g = torch.tensor([[[7.0, 7.0], [0.5, 3.0]], [[100.0, -100.0], [8.0, 8.0]]], dtype=torch.float64)
    A = torch.tensor([0, 1])
    R = torch.tensor([0.0, 3.0], dtype=torch.float64)
    Gam = torch.tensor([1.0, 0.0], dtype=torch.float64)
    w = torch.tensor([2.0, 0.5], dtype=torch.float64)
    loss, td = iqn_loss(theta_t, tau_t, q_next, theta_g, A, R, Gam, kappa, w)
    # row 0: theta = (0, 1), T = (0.5, 3):  u = [[0.5, 3], [-0.5, 2]]
    #   i = 0 (tau .25): .25 * .125 + .25 * 2.5 = .65625 ; i = 1 (tau .5): .5 * .125 + .5 * 1.5 = .8125 ; / N
    row0 = (0.65625 + 0.8125) / 2
    # row 1: theta = (2, 4), T = (3, 3):  u = [[1, 1], [-1, -1]]
    #   i = 0 (tau .1): 2 * .1 * .5 = .1 ; i = 1 (tau .9): 2 * |.9 - 1| * .5 = .1 ; / N
    row1 = (0.1 + 0.1) / 2
    assert math.isclose(float(loss), (2.0 * row0 + 0.5 * row1) / 2, rel_tol=1e-14)
    assert torch.allclose(td, torch.tensor([abs(1.75 - 0.5), abs(3.0 - 3.0)], dtype=torch.float64), atol=1e-15)
    rho, c = quantile_huber_terms(theta_t[0, 0][None], torch.tensor([[0.5, 3.0]], dtype=torch.float64), kappa, tau_t[:1])
    assert torch.allclose(rho, torch.tensor([[0.328125, 0.40625]], dtype=torch.float64), atol=1e-15)
    # c_i = (1/N) sum_j |tau_i - 1{u < 0}| clamp(u):  (.25 * .5 + .25 * 1) / 2,  (.5 * -.5 + .5 * 1) / 2
    assert torch.allclose(c, torch.tensor([[0.1875, 0.125]], dtype=torch.float64), atol=1e-15)


def test_iqn_loss_at_the_midpoints_is_the_quantile_loss():
    g = torch.Generator().manual_seed(0)
    B, A, N = 6, 3, 5
    th_t = torch.randn(B, A, N, generator=g, dtype=torch.float64)
    th_g = torch.randn(B, A, N, generator=g, dtype=torch.float64)
    qn = torch.randn(B, A, generator=g, dtype=torch.float64)
    act = torch.randint(0, A, (B,), generator=g)
    R, Gam = torch.randn(B, generator=g, dtype=torch.float64), torch.full((B,), 0.9, dtype=torch.float64)
    w = torch.rand(B, generator=g, dtype=torch.float64)
    tau = ((2.0 * torch.arange(N, dtype=torch.float64) + 1.0) / (2.0 * N))[None, :].expand(B, N)
    for kappa in (1.0, 0.25):
        a = iqn_loss(th_t, tau, qn, th_g, act, R, Gam, kappa, w)
        b = quantile_huber_loss(th_t, qn, th_g, act, R, Gam, kappa, w)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------- the torch backend against autograd
def _problem(B, A, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)     # noqa: E731
    z_on, z_tg = r(2 * B, 1024), r(B, 1024)
    P = lambda: {"wv": r(1, 512) * 0.05, "bv": r(1), "wa": r(A, 512) * 0.05, "ba": r(A)}   # noqa: E731
    E = lambda: {"wtau": r(1024, 64) * 0.125, "btau": r(1024) * 0.3}     # noqa: E731
    return dict(z_on=z_on, z_tg=z_tg, Pon=P(), Ptg=P(), Eon=E(), Etg=E(),
                act=torch.randint(0, A, (B,), generator=g).to(torch.int32), rew=r(B), isw=torch.rand(B, generator=g,
                                                                                                    dtype=torch.float64),
                gam=torch.tensor([0.0 if i % 3 == 0 else 0.97 for i in range(B)], dtype=torch.float64))


def _theta(h, P, E, tau):
    """The issue's formulas, written out: [rows, A, n]."""
    i = torch.arange(64, dtype=torch.float64)
    c = torch.cos(math.pi * i * tau.double()[..., None])                 # [rows, n, 64]
    phi = torch.relu(c @ E["wtau"].t() + E["btau"])
    x = h[:, None, :] * phi
    v = x[..., :512] @ P["wv"][0] + P["bv"][0]
    adv = x[..., 512:] @ P["wa"].t() + P["ba"]
    return (v[..., None] + adv - adv.mean(-1, keepdim=True)).transpose(1, 2)


@pytest.mark.parametrize("A,N", [(4, 8), (3, 5)])
def test_torch_backend_backward_matches_autograd(A, N):
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    B, kappa, seed, u = 6, 1.0, iqn.iqn_seed(5), 4
    pr = _problem(B, A, N, 10 + A)
    be = TorchBackend(torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                  # noqa: E731
    td, loss, dH, dhead, q = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A)
    taus, ws = torch.zeros(B, 3, N), be.iqn_workspace(B, N, "cpu", torch.float64)
    be.iqn_head(torch.relu(pr["z_on"]), torch.relu(pr["z_tg"]), pr["Pon"], pr["Ptg"], pr["Eon"], pr["Etg"], pr["act"],
                pr["rew"], pr["gam"], pr["isw"], N, kappa, 1.0 / B, seed, torch.tensor([u + 2]), torch.tensor([2]), td, loss,
                dH, dhead, ws, q_out=q, tau_out=taus)
    gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
    be.iqn_wgrad(pr["act"], ws, gr)
    assert torch.equal(taus, iqn.learner_taus(seed, u, B, N))
    # autograd on the definition
    zt = pr["z_on"][:B].clone().requires_grad_(True)
    P = {k: v.clone().requires_grad_(True) for k, v in pr["Pon"].items()}
    E = {k: v.clone().requires_grad_(True) for k, v in pr["Eon"].items()}
    th_t = _theta(torch.relu(zt), P, E, taus[:, 0])
    with torch.no_grad():
        qn = _theta(torch.relu(pr["z_on"][B:]), pr["Pon"], pr["Eon"], taus[:, 1]).mean(-1)
        th_g = _theta(torch.relu(pr["z_tg"]), pr["Ptg"], pr["Etg"], taus[:, 2])
    L, td_ref = iqn_loss(th_t, taus[:, 0], qn, th_g, pr["act"], pr["rew"], pr["gam"], kappa, pr["isw"])
    L.backward()                                                          # mean over the batch = grad_scale 1 / B
    tol = dict(rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(td, td_ref, **tol)
    torch.testing.assert_close(loss.mean(), L.detach(), **tol)
    torch.testing.assert_close(q, th_t.detach().mean(-1), **tol)
    torch.testing.assert_close(dH, zt.grad, **tol)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(gr[k], P[k].grad, **tol)
    torch.testing.assert_close(gr["wtau"], E["wtau"].grad, **tol)
    torch.testing.assert_close(gr["btau"], E["btau"].grad, **tol)
    assert float(E["wtau"].grad.abs().max()) > 0 and float(zt.grad.abs().max()) > 0
    # the dhead layout: column k = g_k, column N + a N + k = g_k ([a = a_b] - 1 / A)
    gk = dhead[:, :N]
    onehot = torch.nn.functional.one_hot(pr["act"].long(), A).double()
    torch.testing.assert_close(dhead[:, N:].reshape(B, A, N), gk[:, None, :] * (onehot - 1.0 / A)[:, :, None], **tol)


def test_consecutive_updates_draw_different_taus():
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    B, A, N = 4, 3, 5
    pr = _problem(B, A, N, 3)
    be = TorchBackend(torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                  # noqa: E731
    ctr, out = torch.zeros(1, dtype=torch.int64), []
    for _ in range(2):
        taus, loss = torch.zeros(B, 3, N), z(B)
        be.iqn_head(torch.relu(pr["z_on"]), torch.relu(pr["z_tg"]), pr["Pon"], pr["Ptg"], pr["Eon"], pr["Etg"], pr["act"],
                    pr["rew"], pr["gam"], None, N, 1.0, 1.0 / B, iqn.iqn_seed(0), ctr, None, z(B), loss, z(B, 1024),
                    z(B, (A + 1) * N), be.iqn_workspace(B, N, "cpu", torch.float64), tau_out=taus)
        out.append((taus, loss))
        ctr += 1
    assert not torch.equal(out[0][0], out[1][0]) and not torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[1][0], iqn.learner_taus(iqn.iqn_seed(0), 1, B, N))
    with pytest.raises(ValueError, match="kappa"):
        be.iqn_head(torch.relu(pr["z_on"]), torch.relu(pr["z_tg"]), pr["Pon"], pr["Ptg"], pr["Eon"], pr["Etg"], pr["act"],
                    pr["rew"], pr["gam"], None, N, 0.0, 1.0 / B, 1, ctr, None, z(B), z(B), z(B, 1024), z(B, (A + 1) * N),
                    be.iqn_workspace(B, N, "cpu", torch.float64))


def test_actor_oracle_midpoints_and_draws():
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    E_, A, K = 5, 3, 4
    pr = _problem(E_, A, K, 8)
    be = TorchBackend(torch.float64)
    h = torch.relu(pr["z_tg"])
    q, a = torch.zeros(E_, A, dtype=torch.float64), torch.zeros(E_, dtype=torch.int32)
    eps, ctr = torch.zeros(E_), torch.zeros(1, dtype=torch.int64)
    be.iqn_actor_head(h, pr["Pon"], pr["Eon"], eps, ctr, 1, 77, None, 0, K, True, q, a)
    mid = iqn.midpoint_taus(K)[None, :].expand(E_, K)
    torch.testing.assert_close(q, _theta(h, pr["Pon"], pr["Eon"], mid).mean(-1), rtol=1e-12, atol=1e-14)
    assert torch.equal(a, q.argmax(1).to(torch.int32))
    taus = torch.zeros(E_, K)
    be.iqn_actor_head(h, pr["Pon"], pr["Eon"], eps, ctr, 1, 77, torch.tensor([6]), 9, K, False, q, a, tau_out=taus)
    assert torch.equal(taus, iqn.stream_taus(77, 64 * 6 + 9, E_, K))
    torch.testing.assert_close(q, _theta(h, pr["Pon"], pr["Eon"], taus).mean(-1), rtol=1e-12, atol=1e-14)


# ------------------------- the fixtures and tolerances of tests/test_gpu_iqn.py
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", F.SHAPES)
def test_gpu_fixture_and_tolerances_hold_on_the_cpu(B, A, N, split):
    """What tests/test_gpu_iqn.py takes for granted, shown by the oracle alone: no near-tie of the online
    next-state q (top-2 gap >= 1e-3, ten times the q tolerance), at most 10 % of the embedding rows with
    near-kink slack, and the fp32 stand-in within a quarter of every tolerance (the factor 4 covers the
    kernel's different summation order)."""
    r = F.oracle(B, A, N, split)
    assert r["gap"] >= 1e-3, r["gap"]
    assert r["kink_share"] <= 0.10, r["kink_share"]
    h = F.run_torch(B, A, N, split, dtype=torch.float32)
    assert torch.equal(h["taus"], r["taus"])
    errs = F.max_errors(h, r)
    assert 4.0 * max(errs.values()) <= 1.0, errs
    F.compare(h, r)


def test_gpu_actor_fixture_has_clear_greedy_actions():
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    A, stream, t = 6, 5, 11
    fx = F.fixture(64, A)
    be = TorchBackend(torch.float64)
    P, Em = {k: v.double() for k, v in fx["Pon"].items()}, {k: v.double() for k, v in fx["Eon"].items()}
    for E_ in (5, 64):
        for K in (1, 32, 64):
            for mid in (False, True):
                q, a = torch.zeros(E_, A, dtype=torch.float64), torch.zeros(E_, dtype=torch.int32)
                be.iqn_actor_head(fx["Hon"][:E_].double(), P, Em, torch.zeros(E_), torch.zeros(1, dtype=torch.int64), 5,
                                  F.seed_q(), torch.tensor([t]), stream, K, mid, q, a)
                top = q.topk(2, dim=1).values
                assert int(((top[:, 0] - top[:, 1]) > 1e-4).sum()) >= E_ - 1, (E_, K, mid)
