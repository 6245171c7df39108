"""Invertible value rescaling of the n-step target (``Runtime.value_rescale``) without a GPU: the host mirror
learner/rescale.py, the loss oracles by hand, the torch backend's four heads against fp64 autograd through the
oracles, the fused learner on the torch backend against the module under autograd, the n-step builders, the
config keys and refusals, checkpoints across the setting, the conditions tests/test_gpu_value_rescale.py takes
for granted of its scalar-head fixtures, and a short CartPole run."""
import math
import os

import numpy as np
import pytest
import torch

import ddqn_fixtures as F
from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import losses as LS
from apex_dqn_amd.learner import rescale as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"}
KEY = "Runtime.value_rescale"
EPS = 1e-3


# the definition as the issue writes it, in plain Python floats (the mirror evaluates an algebraically equal
# form without the cancelling differences)
def _h(x, eps=EPS):
    return math.copysign(math.sqrt(abs(x) + 1.0) - 1.0, x) + eps * x


def _h_inv(y, eps=EPS):
    r = (math.sqrt(1.0 + 4.0 * eps * (abs(y) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    return math.copysign(r * r - 1.0, y) if y != 0 else 0.0


def _T(R, G, y, eps=EPS):
    return _h(R + G * _h_inv(y, eps), eps)


# ------------------------------------------------------------------ 1. mirror
@pytest.mark.parametrize("eps", [1e-3, 1e-2])
def test_mirror_values_round_trip_and_monotone(eps):
    assert float(RS.h(0.0, eps)) == 0.0 and float(RS.h_inv(0.0, eps)) == 0.0
    assert float(RS.h(3.0, eps)) == pytest.approx(1.0 + 3.0 * eps, rel=1e-15)
    assert float(RS.h(-3.0, eps)) == pytest.approx(-(1.0 + 3.0 * eps), rel=1e-15)
    xs = [0.0, 1e-6, 1e-3, 1.0, 50.0, 1e4, 1e6]
    x = torch.tensor([-v for v in xs[1:]] + xs, dtype=torch.float64)
    back = RS.h_inv(RS.h(x, eps), eps)
    assert back.dtype == torch.float64
    rel = ((back - x).abs() / x.abs().clamp_min(1e-300))[x != 0]
    assert float(rel.max()) <= 1e-12, float(rel.max())
    assert float(back[x == 0].abs().max()) == 0.0
    xn = x.numpy()
    np.testing.assert_allclose(RS.h_inv(RS.h(xn, eps), eps), back.numpy(), rtol=1e-14, atol=0)      # numpy as torch
    # against the definition as written, where that form is accurate
    for v in (-1e4, -50.0, -1.0, 1.0, 50.0, 1e4):
        assert float(RS.h(v, eps)) == pytest.approx(_h(v, eps), rel=1e-13)
        assert float(RS.h_inv(v, eps)) == pytest.approx(_h_inv(v, eps), rel=1e-9)
    grid = torch.cat([-torch.logspace(6, -6, 400, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                      torch.logspace(-6, 6, 400, dtype=torch.float64)])
    for f in (RS.h, RS.h_inv):
        y = f(grid, eps)
        assert bool((y[1:] > y[:-1]).all())
    R = torch.tensor([-7.0, 0.0, 0.3, 50.0], dtype=torch.float64)
    assert torch.equal(RS.rescale_target(R, 0.0, torch.full_like(R, 12.5), eps), RS.h(R, eps))
    # dtype-generic: fp32 in, fp32 out
    assert RS.h(torch.ones(2), eps).dtype == torch.float32 and RS.h(np.ones(2, np.float32), np.float32(eps)).dtype == np.float32


def test_check_eps():
    for bad in (0.0, -1e-3, 1.5, float("nan")):
        with pytest.raises(ValueError, match="value_rescale_eps"):
            RS.check_eps(bad)
    assert RS.check_eps(1) == 1.0 and RS.check_eps(1e-3) == 1e-3


# ------------------------------------------------------------------ 2. oracles by hand
def _huber(d, k=1.0):
    return 0.5 * d * d if abs(d) <= k else k * (abs(d) - 0.5 * k)


def test_ddqn_loss_by_hand():
    # rows: plain, terminal, R = 50; the online net picks a* = 1, 0, 2
    q_on_next = torch.tensor([[0.0, 1.0, 0.5], [2.0, 1.0, 0.0], [0.1, 0.2, 0.3]])
    q_tg_next = torch.tensor([[9.0, 2.0, -4.0], [0.7, 5.0, 5.0], [1.0, 1.0, 3.5]])
    q_t = torch.tensor([[1.5, 0.1, 0.2], [0.3, 1.9, 0.1], [4.0, 5.0, 7.0]], requires_grad=True)
    A = torch.tensor([0, 1, 2])
    R = torch.tensor([0.25, -2.0, 50.0])
    G = torch.tensor([0.97, 0.0, 0.97])
    w = torch.tensor([1.0, 0.5, 2.0])
    f32 = lambda v: float(np.float32(v))                                 # noqa: E731
    T = [_T(f32(0.25), f32(0.97), 2.0), _h(-2.0), _T(50.0, f32(0.97), 3.5)]
    assert T[1] == _T(-2.0, 0.0, 0.7)
    qsa = [1.5, f32(1.9), 7.0]
    d = [f32(T[i]) - qsa[i] for i in range(3)]
    assert abs(d[0]) < 1.0 < abs(d[1]) and abs(d[2]) < 1.0                # both Huber branches
    want = sum(float(w[i]) * _huber(d[i]) for i in range(3)) / 3
    loss, td = LS.ddqn_loss(q_t, q_on_next, q_tg_next, A, R, G, w, rescale_eps=EPS)
    assert float(loss.detach()) == pytest.approx(want, rel=1e-6)
    np.testing.assert_allclose(td.numpy(), np.abs(d), rtol=1e-6)
    # R = 50 is learnable: the plain target would sit at 50 + 0.97 * 3.5
    assert 7.0 < T[2] < 7.8
    # off: the expressions and bits of before
    a = LS.ddqn_loss(q_t, q_on_next, q_tg_next, A, R, G, w)
    b = LS.ddqn_loss(q_t, q_on_next, q_tg_next, A, R, G, w, rescale_eps=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(LS.ddqn_targets(q_on_next, q_tg_next, R, G), LS.ddqn_targets(q_on_next, q_tg_next, R, G, None))


@pytest.mark.parametrize("implicit", [False, True])
def test_quantile_losses_by_hand(implicit):
    N, kappa = 2, 1.0
    d = torch.float64
    theta_t = torch.tensor([[[0.0, 1.0], [0.2, 0.4]], [[1.0, 2.0], [-1.0, 0.5]], [[5.0, 7.0], [0.0, 0.0]]], dtype=d,
                           requires_grad=True)
    q_next = torch.tensor([[0.0, 1.0], [1.0, 0.0], [0.0, 1.0]], dtype=d)                   # a* = 1, 0, 1
    th_tg = torch.tensor([[[9.0, 9.0], [0.5, 2.0]], [[3.0, 4.0], [9.0, 9.0]], [[9.0, 9.0], [3.0, 4.0]]], dtype=d)
    A = torch.tensor([1, 0, 0])
    R = torch.tensor([0.25, -2.0, 50.0], dtype=d)
    G = torch.tensor([0.5, 0.0, 0.5], dtype=d)
    w = torch.tensor([1.0, 0.5, 2.0], dtype=d)
    tau = torch.tensor([[0.1, 0.8], [0.3, 0.6], [0.25, 0.75]], dtype=d) if implicit else \
        torch.tensor([[0.25, 0.75]] * 3, dtype=d)
    T = [[_T(0.25, 0.5, 0.5), _T(0.25, 0.5, 2.0)], [_h(-2.0), _h(-2.0)], [_T(50.0, 0.5, 3.0), _T(50.0, 0.5, 4.0)]]
    th = [[0.2, 0.4], [1.0, 2.0], [5.0, 7.0]]
    per, td = [], []
    for b in range(3):
        s = 0.0
        for i in range(N):
            for j in range(N):
                u = T[b][j] - th[b][i]
                s += abs(float(tau[b, i]) - (1.0 if u < 0 else 0.0)) * _huber(u, kappa) / kappa / N
        per.append(float(w[b]) * s)
        td.append(abs(sum(T[b]) / N - sum(th[b]) / N))
    if implicit:
        got = LS.iqn_loss(theta_t, tau, q_next, th_tg, A, R, G, kappa, w, rescale_eps=EPS)
        off = (LS.iqn_loss(theta_t, tau, q_next, th_tg, A, R, G, kappa, w),
               LS.iqn_loss(theta_t, tau, q_next, th_tg, A, R, G, kappa, w, rescale_eps=None))
    else:
        got = LS.quantile_huber_loss(theta_t, q_next, th_tg, A, R, G, kappa, w, rescale_eps=EPS)
        off = (LS.quantile_huber_loss(theta_t, q_next, th_tg, A, R, G, kappa, w),
               LS.quantile_huber_loss(theta_t, q_next, th_tg, A, R, G, kappa, w, rescale_eps=None))
    assert float(got[0].detach()) == pytest.approx(sum(per) / 3, rel=1e-9)
    np.testing.assert_allclose(got[1].numpy(), td, rtol=1e-9)
    # the mean of the transformed samples is not the transform of the mean
    assert abs(td[0] - abs(_T(0.25, 0.5, 1.25) - 0.3)) > 1e-3
    assert torch.equal(off[0][0], off[1][0]) and torch.equal(off[0][1], off[1][1])


def test_c51_by_hand():
    N, vmin, vmax = 3, 0.0, 2.0
    d = torch.float64
    z = [0.0, 1.0, 2.0]
    p = torch.tensor([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8]], dtype=d)
    R = torch.tensor([1.0, 0.5, 50.0], dtype=d)
    G = torch.tensor([0.9, 0.0, 0.9], dtype=d)
    want = []
    clamped = []
    for b in range(3):
        m = [0.0] * N
        for j in range(N):
            t = _T(float(R[b]), float(G[b]), z[j])
            clamped.append(t > vmax)
            bj = (min(max(t, vmin), vmax) - vmin) / 1.0
            for i in range(N):
                m[i] += float(p[b, j]) * max(0.0, 1.0 - abs(bj - i))
        want.append(m)
    assert clamped[:3] == [False, False, True] and all(clamped[6:])       # one atom of row 0 at v_max, row 2 all
    got = LS.c51_project(p, R, G, vmin, vmax, EPS)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(got.sum(-1).numpy(), 1.0, rtol=1e-12)
    hb = _h(0.5)                                                          # terminal: every atom at h(R)
    np.testing.assert_allclose(got[1].numpy(), [1.0 - hb, hb, 0.0], rtol=1e-9, atol=1e-15)
    assert torch.equal(got[2], torch.tensor([0.0, 0.0, 1.0], dtype=d))
    assert torch.equal(LS.c51_project(p, R, G, vmin, vmax), LS.c51_project(p, R, G, vmin, vmax, None))
    # c51_loss passes it on
    logp = torch.log_softmax(torch.tensor([[[0.1, 0.2, 0.3], [0.0, 1.0, 0.0]]] * 3, dtype=d), -1)
    q_next = torch.tensor([[1.0, 0.0]] * 3, dtype=d)
    pt = torch.stack([p, p.flip(-1)], 1)
    A = torch.tensor([0, 1, 0])
    loss, td = LS.c51_loss(logp, q_next, pt, A, R, G, vmin, vmax, None, rescale_eps=EPS)
    lp = logp[torch.arange(3), A]
    assert float(loss) == pytest.approx(float(-(got * lp).sum(-1).mean()), rel=1e-12)
    zt = torch.tensor(z, dtype=d)
    torch.testing.assert_close(td, ((got * zt).sum(-1) - (lp.exp() * zt).sum(-1)).abs(), rtol=1e-12, atol=0)
    a, b = LS.c51_loss(logp, q_next, pt, A, R, G, vmin, vmax), LS.c51_loss(logp, q_next, pt, A, R, G, vmin, vmax, None,
                                                                           rescale_eps=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 3. torch backend vs autograd
B_, A_, N_, HS_ = 5, 3, 5, 512


def _head_inputs(nv, seed=0, dt=torch.float64):
    """Activations, two heads (``nv`` value rows) and the sampled scalars; a terminal row and an R = 50 row."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    Hon, Htg = torch.relu(r(2 * B_, 2 * HS_)), torch.relu(r(B_, 2 * HS_))
    P = lambda: {"wv": (r(nv, HS_) * 0.05).reshape((HS_,) if nv == 1 else (nv, HS_)), "bv": r(nv),     # noqa: E731
                 "wa": r(A_ * nv, HS_) * 0.05, "ba": r(A_ * nv)}
    Pon, Ptg = P(), P()
    act = torch.randint(0, A_, (B_,), generator=g).to(torch.int32)
    rew = r(B_) * 2
    rew[3] = 50.0
    gam = torch.full((B_,), 0.97, dtype=torch.float64)
    gam[1] = 0.0
    isw = torch.rand(B_, generator=g, dtype=torch.float64) + 0.5
    c = lambda t: t.to(dt) if t.is_floating_point() else t              # noqa: E731
    return (c(Hon), c(Htg), {k: c(v) for k, v in Pon.items()}, {k: c(v) for k, v in Ptg.items()}, act, c(rew), c(gam),
            c(isw))


def _leaf(Hon, Pon):
    h = Hon[:B_].clone().double().requires_grad_(True)
    P = {k: v.clone().double().requires_grad_(True) for k, v in Pon.items()}
    return h, P


def _outs(J, dt):
    return (torch.zeros(B_, dtype=dt), torch.zeros(B_, dtype=dt), torch.zeros(B_, 2 * HS_, dtype=dt),
            torch.zeros(B_, J, dtype=dt))


def _check_grads(be, loss, h, P, Hon, td, td_ref, dH, dhead, tol):
    loss.backward()
    torch.testing.assert_close(td.double(), td_ref.double(), **tol)
    torch.testing.assert_close(dH.double(), h.grad * (h.detach() > 0), **tol)
    g = {k: torch.zeros_like(v.detach()).to(dhead.dtype) for k, v in P.items()}
    be.head_wgrad(Hon, dhead, g)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(g[k].double(), P[k].grad.reshape(g[k].shape), **tol)
        assert float(P[k].grad.abs().max()) > 0


def test_torch_backend_scalar_head_vs_autograd():
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend()
    Hon, Htg, Pon, Ptg, act, rew, gam, isw = _head_inputs(1, dt=torch.float32)
    td, loss, dH, dhead = _outs(A_ + 1, torch.float32)
    q = torch.zeros(B_, A_)
    be.head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, True, 2.0, 1.0 / B_, td, loss, dH, dhead, q_out=q, rescale_eps=EPS)
    h, P = _leaf(Hon, Pon)
    d = lambda t: t.double()                                              # noqa: E731
    q_t = be._dueling_q(h, P, torch.float64)
    q_n = be._dueling_q(d(Hon[B_:]), {k: d(v) for k, v in Pon.items()}, torch.float64)
    q_g = be._dueling_q(d(Htg), {k: d(v) for k, v in Ptg.items()}, torch.float64)
    T = RS.rescale_target(d(rew), d(gam), q_g.gather(1, q_n.argmax(1)[:, None]).squeeze(1), EPS)
    delta = T - q_t.gather(1, act.long()[:, None]).squeeze(1)
    lref = (LS.huber(delta, 2.0) * d(isw)).mean()
    assert bool((delta.abs() > 2.0).any()) and bool((delta.abs() < 2.0).any())          # both Huber branches
    tol = dict(rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(loss.double().mean(), lref.detach(), **tol)
    _check_grads(be, lref, h, P, Hon, td, delta.detach().abs(), dH, dhead, tol)
    # the oracle of learner/losses.py is the same function
    l2, td2 = LS.ddqn_loss(q_t.detach().float(), q_n.float(), q_g.float(), act, rew, gam, isw, kappa=2.0, rescale_eps=EPS)
    torch.testing.assert_close(l2.double(), lref.detach(), **tol)
    # the keyword off (None) is the call without it, bit for bit
    o1, o2 = _outs(A_ + 1, torch.float32), _outs(A_ + 1, torch.float32)
    be.head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, True, 1.0, 1.0 / B_, *o1)
    be.head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, True, 1.0, 1.0 / B_, *o2, rescale_eps=None)
    assert all(torch.equal(a, b) for a, b in zip(o1, o2)) and not torch.equal(o1[0], td)


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_torch_backend_wide_heads_vs_autograd(kind):
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float64)
    dt = torch.float64
    Hon, Htg, Pon, Ptg, act, rew, gam, isw = _head_inputs(N_)
    td, loss, dH, dhead = _outs((A_ + 1) * N_, dt)
    h, P = _leaf(Hon, Pon)
    if kind == "quantile":
        be.qr_head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, N_, 1.0, 1.0 / B_, td, loss, dH, dhead, rescale_eps=EPS)
        lref, td_ref = LS.quantile_huber_loss(be._qr_theta(h, P, A_, N_, dt), be._qr_theta(Hon[B_:], Pon, A_, N_, dt).mean(-1),
                                              be._qr_theta(Htg, Ptg, A_, N_, dt), act, rew, gam, 1.0, isw, rescale_eps=EPS)
    else:
        vmin, vmax = -2.0, 5.0
        z = vmin + torch.arange(N_, dtype=dt) * (vmax - vmin) / (N_ - 1)
        # both ends of the support are reached: R = 50 clamps at v_max, a very negative R at v_min
        rew = rew.clone()
        rew[0] = -50.0
        be.c51_head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, N_, vmin, vmax, 1.0 / B_, td, loss, dH, dhead, rescale_eps=EPS)
        lref, td_ref = LS.c51_loss(be._c51_logp(h, P, A_, N_, dt), (be._c51_logp(Hon[B_:], Pon, A_, N_, dt).exp() * z).sum(-1),
                                   be._c51_logp(Htg, Ptg, A_, N_, dt).exp(), act, rew, gam, vmin, vmax, isw, rescale_eps=EPS)
        tz = RS.rescale_target(rew[:, None], gam[:, None], z[None, :], EPS)
        assert bool((tz[3] > vmax).all()) and bool((tz[0] < vmin).all()) and bool(((tz > vmin) & (tz < vmax)).any())
    tol = dict(rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(loss.mean(), lref.detach(), **tol)
    _check_grads(be, lref, h, P, Hon, td, td_ref, dH, dhead, tol)


def test_torch_backend_implicit_head_vs_autograd():
    from apex_dqn_amd.learner.iqn import learner_taus
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float64)
    dt = torch.float64
    Hon, Htg, Pon, Ptg, act, rew, gam, isw = _head_inputs(1)
    g = torch.Generator().manual_seed(9)
    E = lambda: {"wtau": torch.randn(2 * HS_, 64, generator=g, dtype=dt) * 0.1,      # noqa: E731
                 "btau": torch.randn(2 * HS_, generator=g, dtype=dt) * 0.1 + 0.5}
    Eon, Etg = E(), E()
    td, loss, dH, dhead = _outs((A_ + 1) * N_, dt)
    ws = be.iqn_workspace(B_, N_, "cpu", dt)
    ctr, seed_q = torch.tensor([4], dtype=torch.int64), 77
    be.iqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, act, rew, gam, isw, N_, 1.0, 1.0 / B_, seed_q, ctr, None, td, loss, dH,
                dhead, ws, rescale_eps=EPS)
    taus = learner_taus(seed_q, 4, B_, N_)
    h, P = _leaf(Hon, Pon)
    Ew = {k: v.clone().requires_grad_(True) for k, v in Eon.items()}
    th_t = be._iqn_theta(h, P, Ew, taus[:, 0], dt)[0]
    q_n = be._iqn_theta(Hon[B_:], Pon, Eon, taus[:, 1], dt)[0].mean(-1)
    th_g = be._iqn_theta(Htg, Ptg, Etg, taus[:, 2], dt)[0]
    lref, td_ref = LS.iqn_loss(th_t, taus[:, 0], q_n, th_g, act, rew, gam, 1.0, isw, rescale_eps=EPS)
    lref.backward()
    tol = dict(rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(loss.mean(), lref.detach(), **tol)
    torch.testing.assert_close(td, td_ref, **tol)
    torch.testing.assert_close(dH, h.grad * (h.detach() > 0), **tol)
    gr = {k: torch.zeros_like(v.detach()) for k, v in {**Pon, **Eon}.items()}
    be.iqn_wgrad(act, ws, gr)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(gr[k], P[k].grad.reshape(gr[k].shape), **tol)
    for k in ("wtau", "btau"):
        torch.testing.assert_close(gr[k], Ew[k].grad, **tol)
        assert float(Ew[k].grad.abs().max()) > 0


# ------------------------------------------------------------------ 4. fused learner vs the module
def _setup(N=1, A=6, B=8, big=True, **rt):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": dict(ENV, action_dim=A), "Learner": {"replay_sample_size": B},
                                "Runtime": {"grad_clip": 40.0, "network": "nature64", "presample": False,
                                            "num_atoms": N, "value_rescale": True, **rt}})
    rp = GpuReplayShard(400, 400, 600, 4, device="cpu")
    rng = np.random.default_rng(0)
    seqs = rp.append_frames(rng.integers(0, 255, (300, 84, 84), dtype=np.uint8))
    K = 200
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    nx = np.stack([seqs[i + 3:i + 7] for i in range(K)])
    g = np.full(K, 0.97)
    g[::5] = 0.0
    R = rng.normal(size=K) * (30 if big else 3)             # raw, unclipped rewards
    rp.insert(dict(S_t=st, S_tpn=nx, A_t=rng.integers(0, A, K), R=R, Gamma=g, priority=rng.random(K)))
    return cfg, rp


@pytest.mark.parametrize("N,kind,noisy", [(1, "categorical", False), (7, "quantile", False), (1, "categorical", True)])
def test_fused_backward_matches_autograd(N, kind, noisy):
    from apex_dqn_amd.learner import noisy as NZ
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    from apex_dqn_amd.models.flat_params import flat_to_reference_state
    cfg, rp = _setup(N, dist_head=kind, noisy=noisy)
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.rescale_eps == 1e-3 and L.N == N
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    L._seg1()
    L._seg2()
    if noisy:
        T.Q.set_noise(NZ.split_xi(L.xi[0], L.A, N))
        T.Q_target.set_noise(NZ.split_xi(L.xi[1], L.A, N))
    B, S = L.B, L.S
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    assert float(S["rew"].abs().max()) > 10
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref.detach()) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref.detach())))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    for k, p in T.Q.named_parameters():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")
    # and the target is not the plain one: the same batch with the key off gives other priorities
    cfg0, rp0 = _setup(N, dist_head=kind, noisy=noisy)
    cfg0.Runtime.value_rescale = False
    L0 = FusedNatureLearner(cfg0, "cpu", rp0)
    L0._seg1()
    L0._seg2()
    assert torch.equal(L0.S["idx"], S["idx"]) and float((L0.td_abs - L.td_abs).abs().max()) > 1.0


# ------------------------------------------------------------------ 5. n-step builders
def test_nstep_golden_by_hand():
    """The golden of tests/test_nstep_and_actor.py (n = 3, gamma = 0.99, rewards 1, 10, 100, 1000): R = 1 + 9.9 +
    98.01 = 108.91 stays raw, and the priority is |h(R + gamma^3 h^-1(max_a q(S_3))) - q(S_0, A_0)|; then a
    terminal flush, |h(R_j) - q_j| per remaining window entry."""
    from apex_dqn_amd.actors.nstep import NStepBuilder
    b = NStepBuilder(1, 3, 0.99, (1,), np.float32, value_rescale_eps=EPS)
    rewards = [1.0, 10.0, 100.0, 1000.0]
    qs = [[1.5, 0.5], [0.2, 0.1], [0.3, 0.1], [2.5, 7.25]]
    for t in range(4):
        b.step(np.array([[t]], np.float32), np.array([qs[t]]), np.array([0]), np.array([rewards[t]]), np.array([False]),
               np.array([[t + 1]], np.float32))
    out = b.get()
    assert len(out["A_t"]) == 1 and out["S_t"][0, 0] == 0 and out["S_tpn"][0, 0] == 3
    R = 1.0 + 0.99 * 10.0 + 0.99 ** 2 * 100.0
    assert R == pytest.approx(108.91, abs=1e-9)
    assert float(out["R"][0]) == pytest.approx(R, rel=1e-7) and float(out["Gamma"][0]) == pytest.approx(0.99 ** 3)
    want = abs(_T(R, 0.99 ** 3, 7.25) - 1.5)
    assert float(out["priority"][0]) == pytest.approx(want, rel=1e-6)
    assert want < 20 < abs(R + 0.99 ** 3 * 7.25 - 1.5)
    b.step(np.array([[4]], np.float32), np.array([[0.4, 0.0]]), np.array([0]), np.array([-7.0]), np.array([True]),
           np.array([[5]], np.float32))
    out = b.get()
    # (the pending transition of t = 1 completes first, then the three window entries flush)
    assert len(out["A_t"]) == 4 and float(out["Gamma"][0]) > 0 and np.all(out["Gamma"][1:] == 0)
    Rs = [100.0 + 0.99 * 1000.0 + 0.99 ** 2 * -7.0, 1000.0 + 0.99 * -7.0, -7.0]
    np.testing.assert_allclose(out["R"][1:], Rs, rtol=1e-6)
    np.testing.assert_allclose(out["priority"][1:], [abs(_h(Rs[0]) - 0.3), abs(_h(Rs[1]) - 2.5), abs(_h(-7.0) - 0.4)],
                               rtol=1e-6)


def _drive(builders, steps=300, E=6, A=4, seed=0, p_done=0.08):
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        obs, nx = rng.integers(0, 1000, (E, 2)), rng.integers(0, 1000, (E, 2))
        q = (rng.normal(size=(E, A)) * 4).astype(np.float32)
        act = rng.integers(0, A, E)
        r = (rng.normal(size=E) * 40).astype(np.float32)
        d = rng.random(E) < p_done
        for b in builders:
            b.step(obs, q, act, r, d, nx)
    return [b.get() for b in builders]


def test_native_builder_equals_numpy_builder_and_eps_zero_is_the_old_code():
    from apex_dqn_amd.actors.nstep import NStepBuilder, make_nstep_builder
    from apex_dqn_amd.runtime import native
    if not native.available():
        pytest.skip("host runtime library not built")
    E, n = 6, 3
    mk = lambda cls, **kw: cls(E, n, 0.97, (2,), np.int64, 11, **kw)     # noqa: E731
    for eps in (1e-3, 1e-2):
        a, b = _drive([mk(NStepBuilder, value_rescale_eps=eps), mk(native.NativeNStepBuilder, value_rescale_eps=eps)])
        assert len(a["A_t"]) > 1000 and bool((a["Gamma"] == 0).any()) and float(np.abs(a["R"]).max()) > 50
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    outs = _drive([mk(NStepBuilder), mk(NStepBuilder, value_rescale_eps=0.0), mk(native.NativeNStepBuilder),
                   mk(native.NativeNStepBuilder, value_rescale_eps=0.0)])
    for o in outs[1:]:
        for k in o:
            assert np.array_equal(outs[0][k], o[k]), k
    assert not np.array_equal(outs[0]["priority"], a["priority"])
    assert np.array_equal(outs[0]["R"], a["R"])                          # the replay stores raw R either way
    assert make_nstep_builder(E, n, 0.97, (2,), np.int64, value_rescale_eps=1e-3).value_rescale_eps == 1e-3
    for bad in (-1e-3, 1.5):
        for cls in (NStepBuilder, native.NativeNStepBuilder):
            with pytest.raises(ValueError, match="value_rescale_eps"):
                mk(cls, value_rescale_eps=bad)


# ------------------------------------------------------------------ 6. config
def test_config_keys_defaults_and_bundled_config():
    rt = ApexConfig.from_dict({}).Runtime
    assert rt.value_rescale is False and rt.value_rescale_eps == 1e-3 and rt.clip_rewards is True
    assert ApexConfig.from_dict({}).rescale_eps is None
    c = ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"value_rescale": True, "value_rescale_eps": 1e-2,
                                                           "clip_rewards": False}})
    c2 = ApexConfig.from_dict(c.to_dict())
    assert c2.to_dict() == c.to_dict() and c2.rescale_eps == 1e-2 and c2.Runtime.clip_rewards is False
    for ok in (1, 1.0, 1e-6):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"value_rescale_eps": ok}})
    b = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_rescale.json"))
    assert b.Runtime.value_rescale and b.Runtime.clip_rewards is False and b.Runtime.num_atoms == 1 \
        and b.Runtime.optimizer == "adam" and b.rescale_eps == 1e-3
    # it composes with the other options
    ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"value_rescale": True, "noisy": True, "num_atoms": 51,
                                                       "optimizer": "adam", "target_ema_rate": 0.01}})


@pytest.mark.parametrize("rt", [{"value_rescale_eps": 0.0}, {"value_rescale_eps": -1e-3}, {"value_rescale_eps": 1.5},
                                {"value_rescale_eps": True}, {"value_rescale_eps": "1e-3"},
                                {"value_rescale_eps": float("nan")},
                                {"value_rescale": 1}, {"value_rescale": "true"}, {"clip_rewards": 0},
                                {"value_rescale": True, "munchausen": True},
                                {"value_rescale": True, "network": "impala"},
                                {"value_rescale": True, "world_size": 2},
                                {"value_rescale": True, "force_dp": True}])
def test_config_refusals_name_the_key(rt):
    key = "Runtime.clip_rewards" if "clip_rewards" in rt else KEY
    with pytest.raises(ValueError, match=key):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": rt})


def test_learners_refuse():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    from apex_dqn_amd.learner.impala_learner import FusedImpalaLearner
    from apex_dqn_amd.parallel.dist import EmulatedComm
    cfg, rp = _setup()
    with pytest.raises(ValueError, match=KEY):      # the emulated world
        FusedNatureLearner(cfg, "cpu", rp, comm=EmulatedComm(8, 0, torch.device("cpu")))

    class Comm:                                     # a second rank
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match=KEY):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())
    with pytest.raises(ValueError, match=KEY):
        GraphLearner(cfg, "cpu", rp)
    m = _setup()[0]
    m.Runtime.munchausen = True                     # (past the config check)
    with pytest.raises(ValueError, match=KEY):
        FusedNatureLearner(m, "cpu", rp)
    imp = ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"network": "impala"}})
    imp.Runtime.value_rescale = True
    with pytest.raises(ValueError, match=KEY):
        FusedImpalaLearner(imp, "cpu", rp)


def test_clip_rewards_reaches_the_wrapper():
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    assert make_vec_env("fake_ale", "PongNoFrameskip-v4", 2, 6, seed=1).clip is True
    assert make_vec_env("fake_ale", "PongNoFrameskip-v4", 2, 6, seed=1, clip_rewards=False).clip is False
    from apex_dqn_amd.runtime import loops
    for clip in (True, False):
        cfg = ApexConfig.from_dict({"env_conf": dict(ENV, name="PongNoFrameskip-v4"),
                                    "Runtime": {"env_backend": "fake_ale", "clip_rewards": clip, "value_rescale": not clip}})
        g = loops._make_group(cfg, 2, 0, 2, 0)
        assert g.env.clip is clip and g.builder.value_rescale_eps == (0.0 if clip else 1e-3)


# ------------------------------------------------------------------ 7. checkpoints
def test_checkpoints_load_across_the_setting(tmp_path):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    paths = {}
    learners = {}
    for on in (True, False):
        cfg, rp = _setup(big=False)
        cfg.Runtime.value_rescale = on
        L = FusedNatureLearner(cfg, "cpu", rp)
        L.step()
        L.step()
        paths[on] = str(tmp_path / f"rs_{on}.pt")
        L.save(paths[on])
        learners[on] = L
    ck = {on: torch.load(paths[on], weights_only=False) for on in paths}
    assert set(ck[True]) == set(ck[False])                               # no new keys
    assert not torch.equal(learners[True].p32, learners[False].p32)
    for on in (True, False):
        cfg, rp = _setup(big=False)
        cfg.Runtime.value_rescale = not on
        torch.manual_seed(5)
        L2 = FusedNatureLearner(cfg, "cpu", rp)
        assert L2.load(paths[on])
        src = learners[on]
        for a, b in ((src.p32, L2.p32), (src.t32, L2.t32), (src.rms_v, L2.rms_v), (src.pbf, L2.pbf)):
            assert torch.equal(a, b)
        assert L2.num_q_updates == 2 and (L2.rescale_eps is None) == on
        L2.step()


def test_saved_config_records_the_key(tmp_path):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg, rp = _setup(big=False)
    L = FusedNatureLearner(cfg, "cpu", rp)
    path = str(tmp_path / "c.pt")
    L.save(path)
    blob = repr(torch.load(path, weights_only=False))
    assert "value_rescale" in blob


# ------------------------------------------------------------------ 8. fixture conditions (scalar head)
GPU_HEAD_PROBLEMS = [(1, 1), (33, 4), (7, 18)]
GPU_HEAD_CASES = ("plain", "terminal", "big_rewards", "zero_q")
RESCALE_SEED = {(1, 1): 132, (33, 4): 132, (7, 18): 132}


def rescaled_head_oracle(B, A, split, case, eps=EPS, seed=None, dtype=torch.float64):
    """The oracle of tests/ddqn_fixtures.py under the rescaled target: its own head_oracle fed T as the reward
    of a terminal row (G = T + 0 q exactly), T = h(R + Gamma h^-1(q_target[a*])) from the mirror in ``dtype`` on
    the values the kernel sees (eps rounded to fp32 as the launcher passes it).  ``zero_q``: every head
    parameter 0, so every q is 0 and T = h(R)."""
    fx = F.fixture(B, A, 512, split, RESCALE_SEED[(B, A)] if seed is None else seed)
    c = F.case_inputs(fx, "plain" if case == "zero_q" else case)
    if case == "zero_q":
        z = {k: torch.zeros_like(v) for k, v in fx["Pon"].items()}
        c = dict(c, Pon=z, Ptg=z)
    Hon, Htg = F.join64(fx["Hon"], fx["Hon_lo"]), F.join64(fx["Htg"], fx["Htg_lo"])
    r0 = F.head_oracle(Hon, Htg, c["Pon"], c["Ptg"], c["act"], c["rew"], c["gam"], c["isw"], c["huber"], c["kappa"], 1.0 / B)
    e32 = float(np.float32(eps))
    qg = r0["q_g"][torch.arange(B), r0["astar"]]
    if dtype == torch.float64:
        T = RS.rescale_target(c["rew"].double(), c["gam"].double(), qg, e32)
    else:       # the fp32 instance: the q of the fp32 head, the mirror in fp32
        T = RS.rescale_target(c["rew"].float(), c["gam"].float(), qg.float(), np.float32(e32)).double()
    r = F.head_oracle(Hon, Htg, c["Pon"], c["Ptg"], c["act"], T, torch.zeros(B), c["isw"], c["huber"], c["kappa"], 1.0 / B)
    r["gap"], r["T"], r["inputs"] = r0["gap"], T, c
    return r


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A", GPU_HEAD_PROBLEMS)
def test_gpu_fixture_conditions(B, A, split):
    for case in GPU_HEAD_CASES:
        r = rescaled_head_oracle(B, A, split, case)
        if case != "zero_q" and A >= 2:
            assert r["gap"] > F.MARGIN, (case, r["gap"])
        assert r["kmargin"] > F.MARGIN, (case, r["kmargin"])
        assert bool(torch.isfinite(r["td"]).all())
        if case == "plain" and B >= 5:
            d = r["delta"]
            assert bool((d.abs() <= F.KAPPA).any()) and bool((d.abs() > F.KAPPA).any()), "Huber branches"
        if case == "zero_q":
            assert float(r["q"].abs().max()) == 0.0
            torch.testing.assert_close(r["T"], RS.h(r["inputs"]["rew"].double(), float(np.float32(EPS))), rtol=0, atol=0)
        if case == "terminal":
            torch.testing.assert_close(r["T"], RS.h(r["inputs"]["rew"].double(), float(np.float32(EPS))), rtol=0, atol=0)
        # the fp32 instance of the mirror is within a quarter of the GPU file's td tolerance (1e-4 + 1e-4 |td|)
        r32 = rescaled_head_oracle(B, A, split, case, dtype=torch.float32)
        err = (r32["td"] - r["td"]).abs()
        assert bool((err <= 0.25 * (1e-4 + 1e-4 * r["td"].abs())).all()), (case, float(err.max()))

GPU_IQN_PROBLEMS = [(5, 3, 5), (33, 4, 8), (13, 4, 8)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", GPU_IQN_PROBLEMS)
def test_gpu_fixture_conditions_implicit_head(monkeypatch, B, A, N, split):
    """The implicit head's problems of tests/test_gpu_value_rescale.py on tests/iqn_fixtures.py under the rescaled
    target: the top-2 gap of the online next-state q above the scalar fixtures' MARGIN (every row is compared),
    rows on both Huber branches, and the fp32 instance of the oracle within a quarter of every tolerance."""
    import iqn_fixtures as FI
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    orig = TorchBackend.iqn_head
    monkeypatch.setattr(TorchBackend, "iqn_head", lambda self, *a, **kw: orig(self, *a, rescale_eps=EPS, **kw))
    r = FI.run_torch(B, A, N, split)
    assert r["gap"] > F.MARGIN, r["gap"]
    fx = FI.fixture(B, A, split)
    T = RS.rescale_target(fx["rew"].double()[:, None], fx["gam"].double()[:, None], r["th_target"], EPS)
    u = (T[:, :, None] - r["th"][:, None, :]).abs()
    assert bool((u < FI.KAPPA).any()) and bool((u > FI.KAPPA).any())
    torch.testing.assert_close(r["td"], (T.mean(-1) - r["th"].mean(-1)).abs(), rtol=1e-12, atol=1e-12)
    e = FI.max_errors(FI.run_torch(B, A, N, split, dtype=torch.float32), r)
    assert max(e.values()) <= 0.25, e


# ------------------------------------------------------------------ 9. smoke
def test_mlp_torch_learner_and_cartpole_run_stay_bounded():
    """CartPole-v1: reward 1 per step, never clipped, returns up to 500.  With the key on every q the learner
    forms stays at or below h(1 / (1 - gamma)) + kappa: the largest reachable target is T(n-step R, gamma^n,
    y) <= h(1 / (1 - gamma)) whenever y <= h(1 / (1 - gamma)), and one Huber-bounded step past it is at most
    kappa."""
    from apex_dqn_amd.envs.vector_envs import CartPoleVec
    from apex_dqn_amd.actors.nstep import NStepBuilder
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    torch.manual_seed(0)
    gamma, n, E = 0.97, 3, 8
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 50},
                                "Runtime": {"value_rescale": True, "lr": 1e-3, "optimizer": "adam"}})
    T = TorchLearner(cfg, "cpu")
    env = CartPoleVec(E, 0)
    b = NStepBuilder(E, n, gamma, (4,), np.float32, value_rescale_eps=cfg.rescale_eps)
    obs = env.reset()
    rng = np.random.default_rng(0)
    store = []
    bound = float(RS.h(1.0 / (1.0 - gamma), EPS)) + float(cfg.Runtime.huber_delta)
    losses = []
    for t in range(400):
        q = T.q_values(obs).numpy()
        act = np.where(rng.random(E) < 0.3, rng.integers(0, 2, E), q.argmax(1))
        nxt, rew, done, _ = env.step(act)
        b.step(obs, q, act, rew, done, nxt)
        obs = nxt
        out = b.get()
        if out is not None:
            store.append(out)
        if t >= 50 and t % 2 == 0:
            allb = {k: np.concatenate([o[k] for o in store]) for k in store[0]}
            idx = rng.integers(0, len(allb["A_t"]), 32)
            m = T.step({k: allb[k][idx] for k in ("S_t", "S_tpn", "A_t", "R", "Gamma")})
            losses.append(m["loss"])
            assert float(np.max(q)) <= bound, (t, float(np.max(q)), bound)
    assert len(losses) > 100 and np.isfinite(losses).all()
    assert np.isfinite(np.concatenate([o["priority"] for o in store])).all()
