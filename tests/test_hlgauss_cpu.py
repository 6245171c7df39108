"""Histogram-loss (HL-Gauss) target of the categorical dueling head on the CPU: the target row by hand, the loss
and the torch backend's backward against fp64 autograd, the fused learner's whole backward, config, module,
checkpoints, the torch learners, and what tests/test_gpu_hlgauss.py takes for granted about its fixtures and
tolerances (tests/hlg_fixtures.py), shown by the oracle alone."""
import math
import os

import hlg_fixtures as HF
import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import noisy as NZ
from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
from apex_dqn_amd.learner.losses import hl_gauss_loss, hl_gauss_target
from apex_dqn_amd.learner.rescale import rescale_target
from apex_dqn_amd.learner.torch_learner import TorchLearner
from apex_dqn_amd.models.dueling import DuellingDQN, build_network, c51_support
from apex_dqn_amd.models.flat_params import flat_to_reference_state
from apex_dqn_amd.ops.fused_ops import TorchBackend
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(y, v_min, v_max, N, rho=0.75):
    return hl_gauss_target(torch.tensor([y], dtype=F64), v_min, v_max, N, rho)[0]


# ------------------------------------------------------------------ 1. the target row
def test_target_by_hand():
    """N = 3 on [-1, 1]: delta = 1, edges -1.5, -0.5, 0.5, 1.5, sigma = 0.75."""
    y, s = 0.3, 0.75 * math.sqrt(2.0)
    E = [math.erf((e - y) / s) for e in (-1.5, -0.5, 0.5, 1.5)]
    want = torch.tensor([(E[i + 1] - E[i]) / (E[3] - E[0]) for i in range(3)], dtype=F64)
    m = _row(y, -1.0, 1.0, 3)
    torch.testing.assert_close(m, want, rtol=0, atol=1e-15)
    assert abs(float(m.sum()) - 1.0) < 1e-15 and float(m.min()) > 0
    assert m[1] > m[2] > m[0]
    # y on an atom: the row is symmetric about it
    m0 = _row(0.0, -1.0, 1.0, 3)
    assert float(m0[0]) == float(m0[2]) and m0[1] > m0[0]
    m51 = _row(-10.0 + 0.4 * 20, -10.0, 10.0, 51)
    torch.testing.assert_close(m51[:20], m51[21:41].flip(0), rtol=0, atol=1e-13)     # (0.4 is not an fp64 number)


def test_target_sums_to_one_and_keeps_the_mean_in_the_interior():
    """sum_i m_i = 1 everywhere.  The mean sum_i m_i z_i of the binned Gaussian differs from y by the aliasing
    term of the bin grid, at most (delta / pi) exp(-2 pi^2 rho^2) = 1.9e-6 at delta = 0.4, rho = 0.75, plus the
    shift of a Gaussian truncated d = 4 sigma + delta / 2 = 4.67 sigma away, sigma phi(4.67) = 0.3 x 7.4e-6 =
    2.2e-6 (phi the standard normal density) and falling with d: the bound is 5e-6 for y at
    least 4 sigma inside (measured: 2.5e-6).  Within a sigma of an end the mean is biased by up to 0.15 of a
    return unit here, which is why the priority is taken against y."""
    N, lo, hi = 51, -10.0, 10.0
    z = c51_support(N, lo, hi, F64)
    sigma = 0.75 * 0.4
    y = torch.linspace(lo, hi, 4001, dtype=F64)
    m = hl_gauss_target(y, lo, hi, N, 0.75)
    assert float((m.sum(-1) - 1).abs().max()) < 1e-14 and float(m.min()) >= 0
    bias = ((m * z).sum(-1) - y).abs()
    inner = (y >= lo + 4 * sigma) & (y <= hi - 4 * sigma)
    print(f"interior |mean - y| max {float(bias[inner].max()):.2e}, at the ends {float(bias[~inner].max()):.2e}")
    assert float(bias[inner].max()) < 5e-6
    assert 0.05 < float(bias[~inner].max()) < 0.5
    m21 = hl_gauss_target(torch.linspace(lo, hi, 801, dtype=F64), lo, hi, 21, 0.75)
    assert float((m21.sum(-1) - 1).abs().max()) < 1e-14


def test_target_limits_clamp_and_dtype():
    N, lo, hi = 11, 0.0, 5.0
    # a narrow Gaussian is one-hot on the nearest atom
    m = _row(2.2, lo, hi, N, 1e-3)
    assert int(m.argmax()) == 4 and float(m[4]) == 1.0 and float(m.sum()) == 1.0
    # beyond the range: the row of the end, a truncated Gaussian, not one-hot
    for y0, end in ((7.5, hi), (1e9, hi), (-3.0, lo)):
        assert torch.equal(_row(y0, lo, hi, N), _row(end, lo, hi, N))
    top = _row(hi, lo, hi, N)
    assert int(top.argmax()) == N - 1 and 0.5 < float(top[-1]) < 1.0 and float(top[-2]) > 0.1
    # fp32 in, fp32 out: formed in fp64 from the fp32 y and rounded once
    y32 = torch.tensor([0.3, 4.9], dtype=torch.float32)
    m32 = hl_gauss_target(y32, lo, hi, N)
    assert m32.dtype == torch.float32 and torch.equal(m32, hl_gauss_target(y32.double(), lo, hi, N).float())
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma_ratio"):
            _row(1.0, lo, hi, N, bad)


def _loss_inputs(B=6, A=3, N=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)              # noqa: E731
    return dict(logits=r(B, A, N), qn=r(B, A), qg=r(B, A) * 2, act=torch.randint(0, A, (B,), generator=g),
                R=r(B), G=torch.tensor([0.9, 0.0, 0.9, 0.9, 0.0, 0.9], dtype=F64)[:B], w=torch.rand(B, generator=g, dtype=F64))


def test_loss_targets_terminal_rows_and_priority():
    d = _loss_inputs()
    lo, hi, N = -3.0, 3.0, 9
    lp = torch.log_softmax(d["logits"], -1)
    loss, td = hl_gauss_loss(lp, d["qn"], d["qg"], d["act"], d["R"], d["G"], lo, hi, 0.75, d["w"])
    ar = torch.arange(6)
    y = (d["R"] + d["G"] * d["qg"][ar, d["qn"].argmax(1)]).clamp(lo, hi)
    assert torch.equal(y[d["G"] == 0], d["R"][d["G"] == 0].clamp(lo, hi))       # Gamma = 0: y = R
    m = hl_gauss_target(y, lo, hi, N, 0.75)
    want = -(d["w"] * (m * lp[ar, d["act"]]).sum(-1)).mean()
    assert float(loss) == float(want)
    z = c51_support(N, lo, hi, F64)
    torch.testing.assert_close(td, (y - (lp[ar, d["act"]].exp() * z).sum(-1)).abs(), rtol=0, atol=1e-14)
    # value rescaling: one scalar T(R, Gamma, q) replaces the target
    loss_r, td_r = hl_gauss_loss(lp, d["qn"], d["qg"], d["act"], d["R"], d["G"], lo, hi, 0.75, d["w"], rescale_eps=1e-3)
    y_r = rescale_target(d["R"], d["G"], d["qg"][ar, d["qn"].argmax(1)], 1e-3).clamp(lo, hi)
    m_r = hl_gauss_target(y_r, lo, hi, N, 0.75)
    assert float(loss_r) == float(-(d["w"] * (m_r * lp[ar, d["act"]]).sum(-1)).mean())
    torch.testing.assert_close(td_r, (y_r - (lp[ar, d["act"]].exp() * z).sum(-1)).abs(), rtol=0, atol=1e-14)


# ------------------------------------------------------------------ 2. gradients
def test_loss_gradient_is_w_p_minus_m_over_B():
    d = _loss_inputs()
    lo, hi, N, B = -3.0, 3.0, 9, 6
    logits = d["logits"].clone().requires_grad_(True)
    loss, _ = hl_gauss_loss(torch.log_softmax(logits, -1), d["qn"], d["qg"], d["act"], d["R"], d["G"], lo, hi, 0.5, d["w"])
    loss.backward()
    ar = torch.arange(B)
    y = (d["R"] + d["G"] * d["qg"][ar, d["qn"].argmax(1)]).clamp(lo, hi)
    m = hl_gauss_target(y, lo, hi, N, 0.5)
    want = torch.zeros_like(logits)
    want[ar, d["act"]] = d["w"][:, None] * (torch.softmax(d["logits"], -1)[ar, d["act"]] - m) / B
    torch.testing.assert_close(logits.grad, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("rescale_eps", [None, 1e-3])
def test_torch_backend_backward_matches_autograd(rescale_eps):
    """dhead, dH and the head weight gradients of ``TorchBackend.hlg_head`` + ``head_wgrad`` in fp64 against
    autograd through the same head and ``hl_gauss_loss``."""
    B, A, N, HS = 7, 4, 13, 512
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)              # noqa: E731
    pre = r(2 * B, 2 * HS)                                              # (dH carries the stream ReLUs' mask)
    Hon, Htg = torch.relu(pre), torch.relu(r(B, 2 * HS))
    mk = lambda: {"wv": r(N, HS) * 0.05, "bv": r(N), "wa": r(A * N, HS) * 0.05, "ba": r(A * N)}     # noqa: E731
    Pon, Ptg = mk(), mk()
    act = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    rew, gam, isw = r(B) * 3, torch.full((B,), 0.97, dtype=F64), torch.rand(B, generator=g, dtype=F64)
    gam[::3] = 0.0
    be = TorchBackend(F64)
    td, loss, dH, dhead, q = (torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(B, 2 * HS, dtype=F64),
                              torch.zeros(B, (A + 1) * N, dtype=F64), torch.zeros(B, A, dtype=F64))
    be.hlg_head(Hon, Htg, Pon, Ptg, act, rew, gam, isw, N, -10.0, 10.0, 0.75, 1.0 / B, td, loss, dH, dhead, q_out=q,
                rescale_eps=rescale_eps)
    gr = {k: torch.zeros_like(v) for k, v in Pon.items()}
    be.head_wgrad(Hon, dhead, gr)
    # autograd
    P = {k: v.clone().requires_grad_(True) for k, v in Pon.items()}
    x = pre[:B].clone().requires_grad_(True)
    h = torch.relu(x)
    v = h[:, :HS] @ P["wv"].t() + P["bv"]
    a = h[:, HS:] @ P["wa"].t() + P["ba"]
    v.retain_grad()
    a.retain_grad()
    adv = a.reshape(B, A, N)
    lp = torch.log_softmax(v[:, None, :] + adv - adv.mean(1, keepdim=True), -1)
    z = c51_support(N, -10.0, 10.0, F64)
    with torch.no_grad():
        qn = (be._c51_logp(Hon[B:], Pon, A, N, F64).exp() * z).sum(-1)
        qg = (be._c51_logp(Htg, Ptg, A, N, F64).exp() * z).sum(-1)
    ref, td_ref = hl_gauss_loss(lp, qn, qg, act, rew, gam, -10.0, 10.0, 0.75, isw, rescale_eps=rescale_eps)
    ref.backward()
    assert abs(float(ref.detach()) - float(loss.mean())) < 1e-14
    torch.testing.assert_close(td, td_ref, rtol=0, atol=1e-13)
    torch.testing.assert_close(q, (lp.detach().exp() * z).sum(-1), rtol=0, atol=1e-13)
    torch.testing.assert_close(dhead[:, :N], v.grad, rtol=0, atol=1e-15)
    torch.testing.assert_close(dhead[:, N:], a.grad, rtol=0, atol=1e-15)
    torch.testing.assert_close(dH, x.grad, rtol=1e-12, atol=1e-15)
    for k in P:
        torch.testing.assert_close(gr[k], P[k].grad, rtol=1e-12, atol=1e-15)
    assert float(dhead.abs().max()) > 1e-3


def _setup(N, A=6, **rt):
    """tests/test_c51_cpu.py ``_setup`` with the histogram loss."""
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": 8},
                                "Runtime": {"grad_clip": 40.0, "network": "nature64", "presample": False,
                                            "num_atoms": N, "v_min": -10.0, "v_max": 10.0, "dist_head": "hl_gauss",
                                            **rt}})
    rp = GpuReplayShard(400, 400, 600, 4, device="cpu")
    rng = np.random.default_rng(0)
    seqs = rp.append_frames(rng.integers(0, 255, (300, 84, 84), dtype=np.uint8))
    K = 200
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    nx = np.stack([seqs[i + 3:i + 7] for i in range(K)])
    g = np.full(K, 0.97)
    g[::5] = 0.0
    rp.insert(dict(S_t=st, S_tpn=nx, A_t=rng.integers(0, A, K), R=rng.normal(size=K) * 3, Gamma=g,
                   priority=rng.random(K)))
    return cfg, rp


@pytest.mark.parametrize("A,N,rt", [(4, 7, {}), (3, 51, {}), (4, 7, {"noisy": True}), (4, 7, {"value_rescale": True}),
                                    (4, 7, {"hl_gauss_sigma_ratio": 0.25})])
def test_fused_backward_matches_autograd(A, N, rt):
    """The whole hand-written backward of the fused learner (torch backend) against autograd through the module
    and ``hl_gauss_loss``, at tests/test_c51_cpu.py's bounds; with noisy layers the module gets the fused step's
    draws."""
    cfg, rp = _setup(N, A, **rt)
    assert cfg.hl_gauss and not cfg.quantile and not cfg.implicit
    L = FusedNatureLearner(cfg, "cpu", rp)
    assert L.N == N and L.dhead.shape == (8, (A + 1) * N) and not L._defer_fc_epilogue
    T = TorchLearner(cfg, "cpu")
    T.Q.load_state_dict(L.reference_state_dict())
    T.Q_target.load_state_dict(L.reference_state_dict())
    L._seg1()
    L._seg2()
    if rt.get("noisy"):
        T.Q.set_noise(NZ.split_xi(L.xi[0], L.A, N))
        T.Q_target.set_noise(NZ.split_xi(L.xi[1], L.A, N))
    B, S = L.B, L.S
    batch = dict(S_t=L.frames[:B], S_tpn=L.frames[B:2 * B], A_t=S["act"], R=S["rew"], Gamma=S["gam"],
                 weights=S["weights"])
    lref, td = T.compute_loss_and_priorities(batch)
    T.optimizer.zero_grad()
    lref.backward()
    assert abs(float(lref) - float(L.loss_b.mean())) < 1e-5 * max(1.0, abs(float(lref)))
    torch.testing.assert_close(td, L.td_abs, rtol=1e-5, atol=1e-5)
    gf = flat_to_reference_state(L.G, L.c1)
    names = dict(T.Q.named_parameters())
    assert set(gf) == set(names)
    for k, p in names.items():
        torch.testing.assert_close(gf[k], p.grad, rtol=1e-4, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")
    assert float(gf["value.weight"].abs().max()) > 0
    # not the projected cross-entropy: the same learner under "categorical" has another loss
    cfg_c, rp_c = _setup(N, A, **{**rt, "dist_head": "categorical"})
    C = FusedNatureLearner(cfg_c, "cpu", rp_c)
    C._seg1()
    C._seg2()
    assert torch.equal(C.S["idx"], S["idx"]) and not torch.allclose(C.loss_b, L.loss_b)


def test_fused_step_updates_params_and_priorities():
    cfg, rp = _setup(51, optimizer="adam", target_ema_rate=0.01, lr_warmup_steps=2)
    L = FusedNatureLearner(cfg, "cpu", rp)
    p0, t0, leaf0 = L.p32.clone(), L.t32.clone(), rp.leaf.clone()
    L.step()
    o = L.layout.offsets
    assert not torch.equal(p0[o["wv"]:o["wfc"]], L.p32[o["wv"]:o["wfc"]]) and not torch.equal(t0, L.t32)
    idx = L.S["idx"]
    assert not torch.equal(leaf0[idx], rp.leaf[idx])
    assert torch.isfinite(rp.leaf).all() and L.num_q_updates == 1
    with torch.no_grad():
        q = L.q_values(L.frames[:4])
    assert q.shape == (4, 6) and float(q.abs().max()) <= 10.0


# ------------------------------------------------------------------ 3. config, module, learners
def _cfg(**rt):
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Runtime": rt})


HL = dict(num_atoms=51, dist_head="hl_gauss")


@pytest.mark.parametrize("rt,key", [
    (dict(dist_head="hl_gauss"), "num_atoms"), (dict(dist_head="hl-gauss", num_atoms=51), "dist_head"),
    (dict(HL, hl_gauss_sigma_ratio=0.0), "hl_gauss_sigma_ratio"), (dict(HL, hl_gauss_sigma_ratio=-1.0), "hl_gauss_sigma_ratio"),
    (dict(HL, hl_gauss_sigma_ratio=float("inf")), "hl_gauss_sigma_ratio"),
    (dict(HL, hl_gauss_sigma_ratio=float("nan")), "hl_gauss_sigma_ratio"),
    (dict(HL, hl_gauss_sigma_ratio="0.75"), "hl_gauss_sigma_ratio"), (dict(HL, hl_gauss_sigma_ratio=True), "hl_gauss_sigma_ratio"),
    (dict(HL, v_min=3.0, v_max=3.0), "v_min"), (dict(HL, num_atoms=65), "num_atoms"),
    (dict(HL, network="impala"), "num_atoms"), (dict(HL, world_size=2), "num_atoms"), (dict(HL, force_dp=True), "num_atoms"),
    (dict(HL, munchausen=True), "munchausen"),
])
def test_config_refusals(rt, key):
    with pytest.raises(ValueError, match=key):
        _cfg(**rt)


def test_config_accepts_round_trips_and_ignores_the_key_elsewhere():
    c = _cfg(**HL)
    assert c.hl_gauss and c.distributional and not c.quantile and not c.implicit
    assert c.Runtime.hl_gauss_sigma_ratio == 0.75 and c.head_kw()["dist_head"] == "hl_gauss"
    c = ApexConfig.from_dict(_cfg(**HL, hl_gauss_sigma_ratio=2, huber_delta=0.0, loss="mse").to_dict())
    assert c.hl_gauss and c.Runtime.hl_gauss_sigma_ratio == 2            # huber_delta / loss do not apply
    for n in (2, 64):
        assert _cfg(num_atoms=n, dist_head="hl_gauss").hl_gauss
    for kind in ("categorical", "quantile", "implicit"):                 # read only under "hl_gauss"
        assert not _cfg(num_atoms=8, dist_head=kind, hl_gauss_sigma_ratio=-1.0).hl_gauss
    assert not _cfg(hl_gauss_sigma_ratio=0.0).hl_gauss and not _cfg().hl_gauss
    f = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_hlgauss.json"))
    assert f.hl_gauss and f.Runtime.num_atoms == 51 and f.Runtime.optimizer == "adam" and f.network == "nature64"


def test_learners_without_a_distributional_head_refuse():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    cfg, rp = _setup(51)
    with pytest.raises(ValueError, match="num_atoms"):
        GraphLearner(cfg, "cpu", rp)

    class Comm:
        rank, world_size, group = 0, 2, None
    with pytest.raises(ValueError, match="num_atoms"):
        FusedNatureLearner(cfg, "cpu", rp, comm=Comm())


@pytest.mark.parametrize("noisy", [False, True])
def test_module_is_the_categorical_module(noisy):
    A, N = 5, 21
    kw = dict(num_atoms=N, v_min=-4.0, v_max=6.0, noisy=noisy)
    torch.manual_seed(2)
    a = DuellingDQN((4, 84, 84), A, dist_head="hl_gauss", **kw)
    b = DuellingDQN((4, 84, 84), A, dist_head="categorical", **kw)
    assert tuple(a.state_dict().keys()) == tuple(b.state_dict().keys())
    b.load_state_dict(a.state_dict())
    if noisy:
        for net in (a, b):
            net.set_noise(NZ.noise_vectors(3, 0, 0, A, N))
    x = torch.randint(0, 255, (3, 4, 84, 84), dtype=torch.uint8)
    with torch.no_grad():
        for u, v in zip(a(x), b(x)):
            assert torch.equal(u, v)
        assert torch.equal(a.log_probs(x), b.log_probs(x))
        torch.testing.assert_close(a(x)[2], (a.log_probs(x).exp() * c51_support(N, -4.0, 6.0)).sum(-1), rtol=0, atol=0)
    mlp = build_network("mlp", [4], 2, num_atoms=11, v_min=0.0, v_max=5.0, dist_head="hl_gauss")
    assert mlp.log_probs(torch.randn(5, 4)).shape == (5, 2, 11)
    with pytest.raises(ValueError, match="dist_head"):
        DuellingDQN((4, 84, 84), A, num_atoms=N, dist_head="gauss")


def test_checkpoint_kind_mismatch_and_resume_with_another_sigma(tmp_path):
    cfg, rp = _setup(21)
    L = FusedNatureLearner(cfg, "cpu", rp)
    L.step()
    L.step()
    path = str(tmp_path / "hlg.pt")
    L.save(path)
    # resume under another sigma ratio: the state is taken, the next step uses the new sigma
    cfg2, rp2 = _setup(21, hl_gauss_sigma_ratio=1.5)
    torch.manual_seed(5)
    L2 = FusedNatureLearner(cfg2, "cpu", rp2)
    assert not torch.equal(L.p32, L2.p32) and L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m)):
        assert torch.equal(a, b)
    assert L2.num_q_updates == 2
    L2.step()
    assert L2.num_q_updates == 3 and torch.isfinite(L2.loss_b).all()
    # the same shapes under another kind: refused before anything is copied
    for kind in ("categorical", "quantile"):
        cfg3, rp3 = _setup(21, dist_head=kind)
        L3 = FusedNatureLearner(cfg3, "cpu", rp3)
        p3 = L3.p32.clone()
        with pytest.raises(ValueError, match="dist_head"):
            L3.load(path)
        assert torch.equal(p3, L3.p32)
    cfg4, rp4 = _setup(21, dist_head="categorical")
    L4 = FusedNatureLearner(cfg4, "cpu", rp4)
    L4.save(str(tmp_path / "c51.pt"))
    with pytest.raises(ValueError, match="dist_head"):
        L.load(str(tmp_path / "c51.pt"))
    mlp = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Runtime": {"num_atoms": 11, "dist_head": "hl_gauss"}})
    T = TorchLearner(mlp, "cpu")
    T.save(str(tmp_path / "mlp.pt"))
    mlp_c = ApexConfig.from_dict({**mlp.to_dict(), "Runtime": {**mlp.to_dict()["Runtime"], "dist_head": "categorical"}})
    with pytest.raises(ValueError, match="dist_head"):
        TorchLearner(mlp_c, "cpu").load(str(tmp_path / "mlp.pt"))


def test_mlp_torch_learner_trains_on_a_fixed_batch():
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Learner": {"q_target_sync_freq": 1000},
                                "Runtime": {"num_atoms": 11, "v_min": 0.0, "v_max": 10.0, "lr": 1e-3,
                                            "dist_head": "hl_gauss"}})
    T = TorchLearner(cfg, "cpu")
    g = torch.Generator().manual_seed(3)
    B = 32
    batch = dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                 A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g) * 3,
                 Gamma=torch.full((B,), 0.97), weights=torch.rand(B, generator=g) + 0.5)
    first = T.step(batch)
    assert first["td_abs"].shape == (B,) and np.isfinite(first["td_abs"]).all()
    for _ in range(48):
        T.step(batch)
    last = T.step(batch)
    assert T.num_q_updates == 50 and last["loss"] < first["loss"]
    assert float(np.mean(last["td_abs"])) < float(np.mean(first["td_abs"]))
    with torch.no_grad():
        ref, _ = hl_gauss_loss(T.Q.log_probs(batch["S_t"]), T.Q(batch["S_tpn"])[2], T.Q_target(batch["S_tpn"])[2],
                               batch["A_t"], batch["R"], batch["Gamma"], 0.0, 10.0, 0.75, batch["weights"])
        now, _ = T.compute_loss_and_priorities(batch)
    assert float(ref) == float(now)


def test_inline_cartpole_learns():
    """tests/test_learner_runtime.py test_inline_cartpole_learns with the histogram loss on [0, 100] (the
    discounted return of a full episode at gamma = 0.99)."""
    from apex_dqn_amd.runtime.loops import train_inline
    torch.manual_seed(0)
    cfg = ApexConfig.from_dict({
        "env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
        "Actor": {"num_actors": 4, "num_steps": 3, "Q_network_sync_freq": 50, "n_step_transition_batch_size": 8},
        "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 64, "q_target_sync_freq": 100,
                    "remove_old_xp_freq": 50},
        "Replay_Memory": {"soft_capacity": 5000},
        "Runtime": {"lr": 1e-3, "log_every": 100, "num_atoms": 51, "v_min": 0.0, "v_max": 100.0,
                    "dist_head": "hl_gauss"}})
    out = train_inline(cfg, 2500, actor_steps_per_update=1)
    assert out["learner"].num_q_updates == 2500 and np.isfinite(out["losses"]).all()
    assert out["mean_return_last"] > 40  # random policy averages ~22


# ------------------------------------------------------------------ 4. what the GPU file takes for granted
@pytest.mark.parametrize("prob", HF.PROBLEMS, ids=lambda p: "-".join(str(x) for x in p))
def test_gpu_fixture_has_no_near_tie_few_clamped_rows_and_a_close_fp32_stand_in(prob):
    """Every head problem of tests/test_gpu_hlgauss.py, by the oracle alone: the online next-state argmax has no
    near-tie (top-2 gap >= 1e-3), at most one row is clamped where clamping is not the point, and the fp32 torch
    backend -- the CPU stand-in of the kernel, the same fp32 softmax, q and y with the row formed in fp64 -- sits
    within a quarter of every tolerance the GPU file applies."""
    B, A, N, split, case, sigma, eps = prob
    r = HF.oracle(*prob)
    assert r["gap"] >= 1e-3, r["gap"]
    clamped = int(((r["y0"] < HF.VMIN) | (r["y0"] > HF.VMAX)).sum())
    assert clamped == B if case in ("rew_hi", "rew_lo") else clamped <= 1, clamped
    h = HF.run_torch(*prob, dtype=torch.float32)
    e = HF.max_errors(h, r)
    print(prob, f"gap {r['gap']:.2e} clamped {clamped}", {k: f"{v:.2e}" for k, v in e.items()})
    worst = max(v for k, v in e.items() if k != "dhead_abs")
    assert worst <= 0.25, e
    # the measured stand-in error behind DHEAD_ATOL: within a factor of two of what is written down
    assert e["dhead_abs"] <= 2.0 * HF.STANDIN_DHEAD_ERR[(B, sigma)], e["dhead_abs"]
    assert h["isn"] == r["isn"] and h["count"] == r["count"] == B


def test_dhead_tolerance_is_four_times_the_stand_in_error():
    worst = max(HF.STANDIN_DHEAD_ERR.values())
    assert 4.0 * worst <= HF.DHEAD_ATOL < 8.0 * worst
    assert HF.TOL["dhead"] == (1e-4, HF.DHEAD_ATOL)
    # every other tolerance is tests/test_gpu_c51.py _compare's
    assert HF.TOL["td"] == (1e-4, 1e-4) and HF.TOL["loss"] == (1e-4, 1e-5) and HF.TOL["dH"] == (1e-2, 1e-6)
    assert HF.TOL["q"] == (1e-4, 1e-4) and HF.TOL["g"] == (1e-3, 1e-6)
    # C51's 1e-7 would not hold four stand-in errors
    assert 4.0 * HF.STANDIN_DHEAD_ERR[(64, 0.25)] > 1e-7
